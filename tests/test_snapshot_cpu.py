"""The snapshot file of include/rtlfm_snapshot.h on the CPU (no GPU, no handle): what the writer writes is the documented
layout byte for byte, a round trip gives back every bit, every kind of damage is answered with -EILSEQ BEFORE any output
is touched, and a failed write leaves `path` and its directory as they were."""
import ctypes as C
import errno
import os
import resource
import struct

import numpy as np
import pytest

from rtlsdr_amd import build as hipbuild
from rtlsdr_amd import capi
from rtlsdr_amd.capi import RtlfmCfg, RtlfmStreamState

CFG_SIZE, REC_SIZE = C.sizeof(RtlfmCfg), C.sizeof(RtlfmStreamState)
HEADER = 24
EILSEQ, ENOBUFS, ENOENT, EINVAL = -errno.EILSEQ, -errno.ENOBUFS, -errno.ENOENT, -errno.EINVAL


@pytest.fixture(scope="module")
def lib():
    hipbuild.build()
    return capi.load()


def random_cfg(rng) -> RtlfmCfg:
    return RtlfmCfg.from_buffer_copy(rng.integers(0, 256, CFG_SIZE, dtype=np.uint8).tobytes())


def random_records(rng, n):
    """(ctypes array of n records, mutes uint32 [n], the records' bytes): every byte random, the padding included."""
    raw = rng.integers(0, 256, n * REC_SIZE, dtype=np.uint8)
    mutes = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return (RtlfmStreamState * n).from_buffer_copy(raw.tobytes()), mutes, raw.tobytes()


def write(lib, path, cfg, n, recs, mutes):
    return lib.rtlfm_snapshot_write(os.fsencode(path), C.byref(cfg), n, recs, mutes.ctypes.data if mutes is not None else None)


def fnv1a64(b: bytes) -> int:
    h = 0xCBF29CE484222325
    for x in b:
        h = ((h ^ x) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def image(cfg, n, rec_bytes, mutes, magic=b"RTLFMSNP", version=1, cfg_size=CFG_SIZE, rec_size=REC_SIZE, count=None):
    """The file as the header comment lays it out, built here without the library."""
    body = magic + struct.pack("<IIII", version, cfg_size, rec_size, n if count is None else count) + bytes(cfg)
    body += np.asarray(mutes, dtype="<u4").tobytes() + rec_bytes
    return body + struct.pack("<Q", fnv1a64(body))


SENTINEL = 0x5A


def read_guarded(lib, path, cap):
    """rtlfm_snapshot_read / _info into outputs filled with a sentinel; returns (code, info code, every output untouched?)."""
    cfg = (C.c_uint8 * CFG_SIZE)(*([SENTINEL] * CFG_SIZE))
    recs = np.full(max(cap, 1) * REC_SIZE, SENTINEL, dtype=np.uint8)
    mutes = np.full(max(cap, 1), SENTINEL * 0x01010101, dtype=np.uint32)
    n = C.c_int(-77)
    r = lib.rtlfm_snapshot_read(os.fsencode(path), C.cast(cfg, C.POINTER(RtlfmCfg)), recs.ctypes.data, mutes.ctypes.data, cap, C.byref(n))
    cfg2 = (C.c_uint8 * CFG_SIZE)(*([SENTINEL] * CFG_SIZE))
    n2 = C.c_int(-77)
    ri = lib.rtlfm_snapshot_info(os.fsencode(path), C.cast(cfg2, C.POINTER(RtlfmCfg)), C.byref(n2))
    clean = (bytes(cfg) == bytes([SENTINEL]) * CFG_SIZE and (recs == SENTINEL).all() and (mutes == SENTINEL * 0x01010101).all()
             and n.value == -77)
    clean_info = bytes(cfg2) == bytes([SENTINEL]) * CFG_SIZE and n2.value == -77
    return r, ri, clean, clean_info


def assert_refused(lib, path, cap=512):
    r, ri, clean, clean_info = read_guarded(lib, path, cap)
    assert (r, ri) == (EILSEQ, EILSEQ)
    assert clean and clean_info, "a refused file wrote to an output"


@pytest.mark.parametrize("n", [1, 5, 300])
def test_round_trip_and_layout(lib, tmp_path, n):
    rng = np.random.default_rng(100 + n)
    cfg = random_cfg(rng)
    recs, mutes, raw = random_records(rng, n)
    path = tmp_path / "s.snap"
    assert write(lib, path, cfg, n, recs, mutes) == 0
    assert path.read_bytes() == image(cfg, n, raw, mutes)  # the documented layout, byte for byte
    assert sorted(os.listdir(tmp_path)) == ["s.snap"]      # the temporary is gone
    got_cfg, got_n = capi.snapshot_info(path)
    assert got_n == n and bytes(got_cfg) == bytes(cfg)
    out = (RtlfmStreamState * n)()
    out_m = np.zeros(n, dtype=np.uint32)
    out_cfg, out_n = RtlfmCfg(), C.c_int()
    assert lib.rtlfm_snapshot_read(os.fsencode(path), C.byref(out_cfg), out, out_m.ctypes.data, n, C.byref(out_n)) == 0
    assert out_n.value == n and bytes(out) == raw and np.array_equal(out_m, mutes) and bytes(out_cfg) == bytes(cfg)
    # the optional outputs may be NULL, and no mutes means all zero
    assert lib.rtlfm_snapshot_read(os.fsencode(path), None, out, None, n + 3, C.byref(out_n)) == 0 and bytes(out) == raw
    assert lib.rtlfm_snapshot_info(os.fsencode(path), None, None) == 0
    assert write(lib, path, cfg, n, recs, None) == 0  # (over an existing file)
    assert path.read_bytes() == image(cfg, n, raw, np.zeros(n, dtype=np.uint32))


@pytest.fixture(scope="module")
def good():
    rng = np.random.default_rng(7)
    n = 5
    cfg = random_cfg(rng)
    _, mutes, raw = random_records(rng, n)
    return cfg, n, raw, mutes, image(cfg, n, raw, mutes)


SECTIONS = ["magic", "version", "cfg_size", "rec_size", "count", "cfg", "mutes", "records", "checksum"]


def section_bounds(n):
    ends = [8, 12, 16, 20, 24, HEADER + CFG_SIZE, HEADER + CFG_SIZE + 4 * n, HEADER + CFG_SIZE + 4 * n + REC_SIZE * n,
            HEADER + CFG_SIZE + 4 * n + REC_SIZE * n + 8]
    return dict(zip(SECTIONS, zip([0] + ends[:-1], ends)))


def test_the_image_built_here_is_accepted(lib, tmp_path, good):
    cfg, n, raw, mutes, img = good
    p = tmp_path / "g.snap"
    p.write_bytes(img)
    r, ri, _, _ = read_guarded(lib, p, n)
    assert (r, ri) == (0, 0)


@pytest.mark.parametrize("section", SECTIONS)
def test_truncated_after_every_section(lib, tmp_path, good, section):
    _, n, _, _, img = good
    lo, hi = section_bounds(n)[section]
    cut = hi if section != "checksum" else hi - 1  # behind the last section the file is whole: one byte short of the end
    p = tmp_path / "t.snap"
    p.write_bytes(img[:cut])
    assert_refused(lib, p)
    p.write_bytes(img[:lo])  # ... and in front of it (for the magic: an empty file)
    assert_refused(lib, p)


@pytest.mark.parametrize("section", SECTIONS)
def test_one_flipped_byte_in_each_section(lib, tmp_path, good, section):
    _, n, _, _, img = good
    lo, hi = section_bounds(n)[section]
    p = tmp_path / "f.snap"
    for at in sorted({lo, (lo + hi) // 2, hi - 1}):
        for bit in (0x01, 0x80):
            b = bytearray(img)
            b[at] ^= bit
            p.write_bytes(bytes(b))
            assert_refused(lib, p)


def test_wrong_magic_version_sizes_count_with_a_valid_checksum(lib, tmp_path, good):
    """Each wrong field in a file whose checksum is RIGHT for its bytes: refused for the field, not by luck of the sum."""
    cfg, n, raw, mutes, _ = good
    p = tmp_path / "w.snap"
    bad = [dict(magic=b"RTLFMSNQ"), dict(magic=b"RTLPWSNP"), dict(version=0), dict(version=2), dict(version=1 << 24),
           dict(cfg_size=CFG_SIZE + 4), dict(cfg_size=CFG_SIZE - 4), dict(rec_size=REC_SIZE + 4), dict(rec_size=REC_SIZE - 2),
           dict(count=0), dict(count=n + 1), dict(count=n - 1), dict(count=0xFFFFFFFF), dict(count=0x80000000 + n)]
    for kw in bad:
        p.write_bytes(image(cfg, n, raw, mutes, **kw))
        assert_refused(lib, p)
    # a count that matches another, consistent length is a good file of that length - and one record more than its bytes is not
    p.write_bytes(image(cfg, n - 1, raw[:REC_SIZE * (n - 1)], mutes[:n - 1]))
    assert read_guarded(lib, p, n)[0] == 0


def test_trailing_bytes_behind_the_checksum(lib, tmp_path, good):
    _, _, _, _, img = good
    p = tmp_path / "x.snap"
    for extra in (b"\0", b"\n", img[-8:], bytes(REC_SIZE + 4)):
        p.write_bytes(img + extra)
        assert_refused(lib, p)


def test_cap_smaller_than_the_file(lib, tmp_path, good):
    _, n, _, _, img = good
    p = tmp_path / "c.snap"
    p.write_bytes(img)
    for cap in (0, 1, n - 1):
        r, ri, clean, _ = read_guarded(lib, p, cap)
        assert r == ENOBUFS and ri == 0 and clean
    assert read_guarded(lib, p, -1)[0] == EINVAL
    assert read_guarded(lib, tmp_path / "nothing.snap", n)[:2] == (ENOENT, ENOENT)
    assert read_guarded(lib, tmp_path, n)[0] < 0  # a directory is no snapshot


def test_write_into_a_missing_directory_leaves_nothing(lib, tmp_path):
    rng = np.random.default_rng(1)
    recs, mutes, _ = random_records(rng, 3)
    assert write(lib, tmp_path / "no_such_dir" / "s.snap", random_cfg(rng), 3, recs, mutes) == ENOENT
    assert os.listdir(tmp_path) == []
    assert write(lib, tmp_path / "s.snap", random_cfg(rng), 0, recs, mutes) == EINVAL
    assert lib.rtlfm_snapshot_write(os.fsencode(tmp_path / "s.snap"), None, 3, recs, None) == EINVAL
    assert os.listdir(tmp_path) == []


def test_a_failed_write_keeps_the_old_file(lib, tmp_path):
    """The write fails half way (the file size limit is hit after the first pages of the temporary): the file at `path` is
    the old one, bit for bit, and the temporary is gone."""
    rng = np.random.default_rng(2)
    cfg = random_cfg(rng)
    recs1, mutes1, raw1 = random_records(rng, 1)
    path = tmp_path / "s.snap"
    assert write(lib, path, cfg, 1, recs1, mutes1) == 0
    before = path.read_bytes()
    recs, mutes, _ = random_records(rng, 300)  # 100 KB
    soft, hard = resource.getrlimit(resource.RLIMIT_FSIZE)
    resource.setrlimit(resource.RLIMIT_FSIZE, (8192, hard))  # (python ignores SIGXFSZ: write() fails with EFBIG)
    try:
        r = write(lib, path, cfg, 300, recs, mutes)
    finally:
        resource.setrlimit(resource.RLIMIT_FSIZE, (soft, hard))
    assert r == -errno.EFBIG
    assert path.read_bytes() == before == image(cfg, 1, raw1, mutes1)
    assert os.listdir(tmp_path) == ["s.snap"]
    assert write(lib, path, cfg, 300, recs, mutes) == 0 and capi.snapshot_info(path)[1] == 300  # and it works again


def test_strerror_has_a_text_for_every_new_code(lib):
    texts = {c: capi.strerror(c) for c in (-errno.ERANGE, -errno.EMEDIUMTYPE, EILSEQ, -errno.EXDEV)}
    assert "number of streams" in texts[-errno.ERANGE] and "configuration" in texts[-errno.EMEDIUMTYPE]
    assert "damaged" in texts[EILSEQ] and "different devices" in texts[-errno.EXDEV]
    assert len(set(texts.values())) == 4
