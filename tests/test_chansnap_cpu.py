"""The channel snapshot of include/rtlfm_chansnap.h on the CPU (no GPU, no handle): what the writer writes is the documented
layout byte for byte, a round trip gives back every bit, every kind of damage is answered with -EILSEQ BEFORE any output is
touched, a failed write leaves `path` and its directory as they were, the two snapshot kinds refuse each other's files, and
the reader survives tools/chansnap_fuzz.cpp under AddressSanitizer + UBSan (a stand-alone program: nothing loaded into
Python runs under a sanitizer)."""
import ctypes as C
import errno
import os
import resource
import struct
import subprocess

import numpy as np
import pytest

from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi
from rtlsdr_amd.capi import RtlfmCfg, RtlfmStreamState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG_SIZE, REC_SIZE = C.sizeof(RtlfmCfg), C.sizeof(RtlfmStreamState)
HEADER = 68
HIST, PIECES = 4096, 16
EILSEQ, ENOBUFS, ENOENT, EINVAL = -errno.EILSEQ, -errno.ENOBUFS, -errno.ENOENT, -errno.EINVAL
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return capi.load()


def fnv1a64(b: bytes) -> int:
    h = 0xCBF29CE484222325
    for x in b:
        h = ((h ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def contents(rng, sources, per, fir=0, K=0, bank_ntaps=0, source_dc=False):
    """Random contents of one file: every byte random, the records' padding included."""
    n = sources * per
    hist = fir > 0 or K > 0
    return dict(
        n=n, per=per, pos=int(rng.integers(0, 1 << 63)), source_dc=source_dc,
        cfg=rng.integers(0, 256, CFG_SIZE, dtype=np.uint8).tobytes(),
        steps=rng.integers(0, 1 << 32, n, dtype=np.uint64).astype("<u4"),
        fir_taps=rng.integers(-32768, 32768, fir).astype("<i2"), fir_shift=int(rng.integers(0, 31)) if fir else 0,
        K=K, bank_taps=rng.integers(-32768, 32768, bank_ntaps if K else 0).astype("<i2"), bank_shift=int(rng.integers(0, 31)) if K else 0,
        bins=rng.integers(0, K, n).astype("<i4") if K else np.zeros(0, "<i4"),
        recs=rng.integers(0, 256, n * REC_SIZE, dtype=np.uint8).tobytes(),
        hist=rng.integers(0, 256, sources * 2 * HIST if hist else 0, dtype=np.uint8),
        dc=rng.integers(0, 1 << 32, sources * PIECES if hist and source_dc else 0, dtype=np.uint64).astype("<u4"))


def image(c, **over):
    """The file as the header comment lays it out, built here without the library.  `over` replaces header fields."""
    hist = len(c["fir_taps"]) > 0 or c["K"] > 0
    f = dict(magic=b"RTLFMCHN", version=1, cfg_size=CFG_SIZE, rec_size=REC_SIZE, n=c["n"], per=c["per"],
             flags=(1 if c["source_dc"] else 0) | (2 if hist else 0), pos=c["pos"], fir_ntaps=len(c["fir_taps"]), fir_shift=c["fir_shift"],
             K=c["K"], bank_ntaps=len(c["bank_taps"]), bank_shift=c["bank_shift"], hist_samples=HIST, dc_pieces=PIECES)
    f.update(over)
    body = f["magic"] + struct.pack("<IIIIIIQIIIIIII", f["version"], f["cfg_size"], f["rec_size"], f["n"], f["per"], f["flags"], f["pos"],
                                    f["fir_ntaps"], f["fir_shift"], f["K"], f["bank_ntaps"], f["bank_shift"], f["hist_samples"], f["dc_pieces"])
    assert len(body) == HEADER
    body += c["cfg"] + c["steps"].tobytes() + c["fir_taps"].tobytes() + c["bank_taps"].tobytes() + c["bins"].tobytes() + c["recs"]
    body += c["hist"].tobytes() + c["dc"].tobytes()
    return body + struct.pack("<Q", fnv1a64(body))


def write(lib, path, c, dc=True):
    recs = (RtlfmStreamState * c["n"]).from_buffer_copy(c["recs"])
    capi.chansnap_write(path, RtlfmCfg.from_buffer_copy(c["cfg"]), c["per"], c["pos"], c["steps"], recs, fir_taps=c["fir_taps"],
                        fir_shift=c["fir_shift"], bank_K=c["K"], bank_taps=c["bank_taps"], bank_shift=c["bank_shift"],
                        bins=c["bins"] if c["K"] else None, hist=c["hist"] if c["hist"].size else None,
                        dc=c["dc"] if dc and c["dc"].size else None, source_dc=c["source_dc"])


def guarded(c, short=None):
    """Output buffers of exactly the file's sizes (`short`: that one an element smaller), filled with a sentinel."""
    sizes = dict(steps=(c["n"], np.uint32), fir_taps=(len(c["fir_taps"]), np.int16), bank_taps=(len(c["bank_taps"]), np.int16),
                 bins=(len(c["bins"]), np.int32), states=(c["n"] * REC_SIZE, np.uint8), hist=(c["hist"].size, np.uint8), dc=(c["dc"].size, np.uint32))
    bufs = {"cfg": np.full(CFG_SIZE, SENTINEL, np.uint8), "hdr": np.full(C.sizeof(capi.RtlfmChansnapHdr), SENTINEL, np.uint8)}
    b = capi.RtlfmChansnapBufs(cfg=bufs["cfg"].ctypes.data)
    for k, (size, dt) in sizes.items():
        cap = size // REC_SIZE if k == "states" else size
        if k == short:
            cap -= 1
        bufs[k] = np.frombuffer(bytes([SENTINEL]) * (max(size, 1) * np.dtype(dt).itemsize), dtype=dt).copy()
        setattr(b, k, bufs[k].ctypes.data)
        setattr(b, "cap_" + k, cap)
    return b, bufs


def untouched(bufs):
    return all((a.view(np.uint8) == SENTINEL).all() for a in bufs.values())


def read_guarded(lib, path, c, short=None):
    """rtlfm_chansnap_read / _info into guarded outputs: (code, info code, every output untouched?, outputs)."""
    b, bufs = guarded(c, short)
    r = lib.rtlfm_chansnap_read(os.fsencode(path), C.cast(bufs["hdr"].ctypes.data, C.POINTER(capi.RtlfmChansnapHdr)), C.byref(b))
    ih = np.full(C.sizeof(capi.RtlfmChansnapHdr), SENTINEL, np.uint8)
    ic = np.full(CFG_SIZE, SENTINEL, np.uint8)
    ri = lib.rtlfm_chansnap_info(os.fsencode(path), C.cast(ih.ctypes.data, C.POINTER(capi.RtlfmChansnapHdr)),
                                 C.cast(ic.ctypes.data, C.POINTER(RtlfmCfg)))
    return r, ri, untouched(bufs) and (ri == 0 or untouched({"h": ih, "c": ic})), bufs


def assert_refused(lib, path, c):
    r, ri, clean, _ = read_guarded(lib, path, c)
    assert (r, ri) == (EILSEQ, EILSEQ)
    assert clean, "a refused file wrote to an output"


# {filter, bank, neither} x {source_dc}; an odd tap count among them (sections behind it are unaligned), a filter AND a bank
COMBOS = [dict(), dict(source_dc=True), dict(fir=33), dict(fir=33, source_dc=True), dict(K=4, bank_ntaps=40), dict(K=16, bank_ntaps=41, source_dc=True),
          dict(fir=7, K=8, bank_ntaps=9, source_dc=True), dict(fir=1024, K=256, bank_ntaps=4096)]


@pytest.mark.parametrize("combo", range(len(COMBOS)))
def test_round_trip_and_layout(lib, tmp_path, combo):
    rng = np.random.default_rng(200 + combo)
    c = contents(rng, 3, 1 if COMBOS[combo].get("K", 0) == 0 and combo % 2 else 2, **COMBOS[combo])
    path = tmp_path / "c.chn"
    write(lib, path, c)
    img = image(c)
    assert path.read_bytes() == img                      # the documented layout, byte for byte
    assert sorted(os.listdir(tmp_path)) == ["c.chn"]     # the temporary is gone
    hdr, cfg = capi.chansnap_info(path)
    assert bytes(cfg) == c["cfg"]
    assert (hdr.nstreams, hdr.per_source, hdr.pos, hdr.fir_ntaps, hdr.fir_shift, hdr.bank_K, hdr.bank_ntaps, hdr.bank_shift, hdr.hist_samples,
            hdr.dc_pieces) == (c["n"], c["per"], c["pos"], len(c["fir_taps"]), c["fir_shift"], c["K"], len(c["bank_taps"]), c["bank_shift"], HIST, PIECES)
    got = capi.chansnap_read(path)
    assert bytes(got["cfg"]) == c["cfg"] and bytes(got["states"]) == c["recs"] and bytes(got["hdr"]) == bytes(hdr)
    for k in ("steps", "fir_taps", "bank_taps", "bins", "hist", "dc"):
        assert np.array_equal(got[k].ravel(), c[k]), k
    # exact caps are enough, one element less in any non-empty section is -ENOBUFS and writes nothing
    r, ri, _, bufs = read_guarded(lib, path, c)
    assert (r, ri) == (0, 0) and bufs["states"].tobytes() == c["recs"]
    for k in ("steps", "fir_taps", "bank_taps", "bins", "states", "hist", "dc"):
        if (c["n"] if k in ("steps", "states") else len(c[k])) == 0:
            continue
        r, ri, clean, _ = read_guarded(lib, path, c, short=k)
        assert (r, ri) == (ENOBUFS, 0) and clean, k
    # every output is optional
    assert lib.rtlfm_chansnap_read(os.fsencode(path), None, C.byref(capi.RtlfmChansnapBufs())) == 0
    assert lib.rtlfm_chansnap_info(os.fsencode(path), None, None) == 0


def test_no_biases_given_means_none_subtracted(lib, tmp_path):
    c = contents(np.random.default_rng(3), 2, 2, fir=5, source_dc=True)
    write(lib, tmp_path / "d.chn", c, dc=False)
    assert (capi.chansnap_read(tmp_path / "d.chn")["dc"] == 0x007F007F).all()


@pytest.fixture(scope="module")
def good():
    c = contents(np.random.default_rng(7), 2, 2, fir=3, K=4, bank_ntaps=5, source_dc=True)
    return c, image(c)


def section_bounds(c):
    names = ["magic", "version", "cfg_size", "rec_size", "n", "per_source", "flags", "pos", "fir_ntaps", "fir_shift", "K", "bank_ntaps", "bank_shift",
             "hist_samples", "dc_pieces", "cfg", "steps", "fir_taps", "bank_taps", "bins", "records", "history", "biases", "checksum"]
    lens = [8, 4, 4, 4, 4, 4, 4, 8, 4, 4, 4, 4, 4, 4, 4, CFG_SIZE, 4 * c["n"], 2 * len(c["fir_taps"]), 2 * len(c["bank_taps"]), 4 * len(c["bins"]),
            len(c["recs"]), c["hist"].size, 4 * c["dc"].size, 8]
    ends = np.cumsum(lens).tolist()
    return dict(zip(names, zip([0] + ends[:-1], ends)))


def test_the_image_built_here_is_accepted(lib, tmp_path, good):
    c, img = good
    assert section_bounds(c)["checksum"][1] == len(img)
    p = tmp_path / "g.chn"
    p.write_bytes(img)
    r, ri, _, bufs = read_guarded(lib, p, c)
    assert (r, ri) == (0, 0) and bufs["hist"].tobytes() == c["hist"].tobytes() and bufs["dc"].tobytes() == c["dc"].tobytes()


def test_one_flipped_byte_in_every_section(lib, tmp_path, good):
    c, img = good
    p = tmp_path / "f.chn"
    for name, (lo, hi) in section_bounds(c).items():
        for at in sorted({lo, (lo + hi) // 2, hi - 1}):
            for bit in (0x01, 0x80):
                b = bytearray(img)
                b[at] ^= bit
                p.write_bytes(bytes(b))
                assert_refused(lib, p, c)


def test_every_header_field_out_of_range_under_a_valid_checksum(lib, tmp_path, good):
    """Each wrong field in a file whose checksum is RIGHT for its bytes: refused for the field, not by luck of the sum."""
    c, _ = good
    p = tmp_path / "w.chn"
    bad = [dict(magic=b"RTLFMSNP"), dict(magic=b"RTLFMCHM"), dict(version=0), dict(version=2), dict(version=1 << 24),
           dict(cfg_size=CFG_SIZE + 4), dict(cfg_size=CFG_SIZE - 4), dict(rec_size=REC_SIZE + 4), dict(rec_size=REC_SIZE - 2),
           dict(n=0), dict(n=c["n"] + 2), dict(n=c["n"] - 2), dict(n=0xFFFFFFFE), dict(n=0x80000000 + c["n"]),
           dict(per=0), dict(per=3), dict(per=c["n"] + 1), dict(per=0xFFFFFFFF),
           dict(flags=1), dict(flags=2), dict(flags=7), dict(flags=0x80000003),
           dict(fir_ntaps=1025), dict(fir_ntaps=0xFFFFFFFF), dict(fir_ntaps=4), dict(fir_shift=31), dict(fir_shift=0xFFFFFFFF),
           dict(K=2), dict(K=3), dict(K=6), dict(K=512), dict(K=0), dict(K=0x80000000),
           dict(bank_ntaps=0), dict(bank_ntaps=4097), dict(bank_ntaps=0xFFFFFFFF), dict(bank_shift=31),
           dict(hist_samples=4095), dict(hist_samples=8192), dict(hist_samples=0), dict(dc_pieces=15), dict(dc_pieces=0)]
    for kw in bad:
        p.write_bytes(image(c, **kw))
        assert_refused(lib, p, c)
    # a filter's shift without a filter, a bank's taps without a bank
    for kw in (dict(fir=0, K=4, bank_ntaps=5), dict(fir=3)):
        c2 = contents(np.random.default_rng(8), 2, 2, **kw)
        p.write_bytes(image(c2))
        assert read_guarded(lib, p, c2)[:2] == (0, 0)
        p.write_bytes(image(c2, **(dict(fir_shift=1) if "K" in kw else dict(bank_ntaps=2))))
        assert_refused(lib, p, c2)
    # a bin outside [0, K), negative or not
    for v in (c["K"], -1, 1 << 30):
        c2 = dict(c, bins=c["bins"].copy())
        c2["bins"][c["n"] - 1] = v
        p.write_bytes(image(c2))
        assert_refused(lib, p, c)


def test_truncated_at_every_length_and_a_byte_appended(lib, tmp_path):
    c = contents(np.random.default_rng(9), 1, 1)  # the smallest file there is: no history
    img = image(c)
    p = tmp_path / "t.chn"
    for cut in range(len(img)):
        p.write_bytes(img[:cut])
        assert_refused(lib, p, c)
    p.write_bytes(img)
    assert read_guarded(lib, p, c)[:2] == (0, 0)
    for extra in (b"\0", b"\n", img[-8:]):
        p.write_bytes(img + extra)
        assert_refused(lib, p, c)
    # with a history: cut in front of and behind every section
    c, img = contents(np.random.default_rng(10), 1, 2, fir=3, source_dc=True), None
    img = image(c)
    for lo, hi in section_bounds(c).values():
        for cut in {lo, hi - 1}:
            p.write_bytes(img[:cut])
            assert_refused(lib, p, c)


def test_the_two_kinds_refuse_each_other(lib, tmp_path, good):
    c, img = good
    p = tmp_path / "k.chn"
    p.write_bytes(img)
    out = (RtlfmStreamState * 64)()
    n = C.c_int(-77)
    assert lib.rtlfm_snapshot_read(os.fsencode(p), None, out, None, 64, C.byref(n)) == EILSEQ and n.value == -77
    assert lib.rtlfm_snapshot_info(os.fsencode(p), None, None) == EILSEQ
    s = tmp_path / "k.snap"
    recs = (RtlfmStreamState * 4)()
    assert lib.rtlfm_snapshot_write(os.fsencode(s), C.byref(RtlfmCfg.default()), 4, recs, None) == 0
    assert_refused(lib, s, c)
    assert read_guarded(lib, tmp_path / "nothing.chn", c)[:2] == (ENOENT, ENOENT)
    assert read_guarded(lib, tmp_path, c)[0] < 0  # a directory is no snapshot


def test_a_write_that_cannot_be_renamed_leaves_nothing(lib, tmp_path):
    """`path` names a directory that is not empty: the temporary is written beside it, rename() fails, and afterwards the
    directory holds what it held - no temporary, no partial file.  The same for a directory that does not exist and for
    what the writer refuses before it opens anything."""
    c = contents(np.random.default_rng(11), 2, 2, fir=3)
    target = tmp_path / "c.chn"
    target.mkdir()
    (target / "keep").write_bytes(b"x")
    with pytest.raises(capi.RtlfmError) as e:
        write(lib, target, c)
    assert e.value.code in (-errno.EISDIR, -errno.ENOTEMPTY, -errno.EEXIST)
    assert sorted(os.listdir(tmp_path)) == ["c.chn"] and os.listdir(target) == ["keep"]
    with pytest.raises(capi.RtlfmError) as e:
        write(lib, tmp_path / "no_such_dir" / "c.chn", c)
    assert e.value.code == ENOENT and sorted(os.listdir(tmp_path)) == ["c.chn"]
    for bad in (dict(K=4, bins=np.array([0, 1, 2, 4], "<i4"), bank_taps=np.ones(3, "<i2")), dict(K=5, bins=np.zeros(4, "<i4"), bank_taps=np.ones(3, "<i2")), dict(fir_shift=31)):
        with pytest.raises(capi.RtlfmError) as e:
            write(lib, tmp_path / "b.chn", dict(c, **bad))
        assert e.value.code == EINVAL
    assert sorted(os.listdir(tmp_path)) == ["c.chn"]


def test_a_failed_write_keeps_the_old_file(lib, tmp_path):
    c1 = contents(np.random.default_rng(12), 1, 1)
    path = tmp_path / "c.chn"
    write(lib, path, c1)
    before = path.read_bytes()
    c2 = contents(np.random.default_rng(13), 4, 2, fir=3)  # 32 KB of history
    soft, hard = resource.getrlimit(resource.RLIMIT_FSIZE)
    resource.setrlimit(resource.RLIMIT_FSIZE, (8192, hard))  # (python ignores SIGXFSZ: write() fails with EFBIG)
    try:
        with pytest.raises(capi.RtlfmError) as e:
            write(lib, path, c2)
    finally:
        resource.setrlimit(resource.RLIMIT_FSIZE, (soft, hard))
    assert e.value.code == -errno.EFBIG
    assert path.read_bytes() == before == image(c1) and os.listdir(tmp_path) == ["c.chn"]
    write(lib, path, c2)
    assert path.read_bytes() == image(c2)


def test_strerror_names_the_new_meanings(lib):
    assert "rtlfm_gpu_channels_load" in capi.strerror(EILSEQ) and "RTLFMCHN" in capi.strerror(EILSEQ)
    assert "rtlfm_gpu_channels_move" in capi.strerror(-errno.EXDEV) and "per_source" in capi.strerror(-errno.EMEDIUMTYPE)
    assert "rtlfm_gpu_load" in capi.strerror(-errno.ENOTSUP) and "rtlfm_gpu_channels_history_get" in capi.strerror(-errno.ENODATA)


def test_new_symbols_are_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "rtlfm_chansnap.h")).read()
    import re
    declared = sorted(set(re.findall(r"\b(rtlfm_chansnap_[a-z_0-9]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))))
    assert declared == sorted(capi.DECLARED_CHANSNAP_SYMBOLS) and len(declared) == 3
    for name in declared + ["rtlfm_gpu_channels_history_get", "rtlfm_gpu_channels_history_set", "rtlfm_gpu_channels_move",
                            "rtlfm_gpu_channels_save", "rtlfm_gpu_channels_load"]:
        assert hasattr(lib, name), name


def test_reader_under_sanitizers(tmp_path):
    """tools/chansnap_fuzz.cpp with chansnap.cpp and snapshot.cpp, AddressSanitizer + UBSan, as a program of its own."""
    exe = tmp_path / "chansnap_fuzz"
    csrc = os.path.join(ROOT, "rtlsdr_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-o", str(exe), os.path.join(ROOT, "tools", "chansnap_fuzz.cpp"), os.path.join(csrc, "chansnap.cpp"),
                           os.path.join(csrc, "snapshot.cpp")])
    r = subprocess.run([str(exe), "20260202", "1500"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "chansnap_fuzz: ok" in r.stdout
