"""RTLSDR_FILE_LIST: the file-backed device layer with one device per line of a list (raw IQ files,
rtl_sdr -H WAV files, tcp://host:port), each device independent of the others, and the usage
rules of rtl_fm_hip -N that are checked before any device is opened or GPU handle created."""
import ctypes as C
import os
import socket
import subprocess
import threading

import numpy as np
import pytest

from rtlsdr_amd import build as hipbuild

CB = C.CFUNCTYPE(None, C.POINTER(C.c_ubyte), C.c_uint32, C.c_void_p)


@pytest.fixture(scope="module")
def shim():
    so, _ = hipbuild.build_host()
    lib = C.CDLL(so)
    lib.rtlsdr_open.argtypes = [C.POINTER(C.c_void_p), C.c_uint32]
    lib.rtlsdr_close.argtypes = [C.c_void_p]
    lib.rtlsdr_read_sync.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    lib.rtlsdr_read_async.argtypes = [C.c_void_p, CB, C.c_void_p, C.c_uint32, C.c_uint32]
    lib.rtlsdr_cancel_async.argtypes = [C.c_void_p]
    lib.rtlsdr_get_device_name.restype = C.c_char_p
    lib.rtlsdr_get_device_name.argtypes = [C.c_uint32]
    lib.rtlsdr_get_device_usb_strings.argtypes = [C.c_uint32, C.c_char_p, C.c_char_p, C.c_char_p]
    return lib


def _wav(payload: bytes) -> bytes:
    """What rtl_sdr -H writes, in shape: RIFF/WAVE, a fmt chunk, an odd-sized chunk the reader must step over, data."""
    fmt = (1).to_bytes(2, "little") + (2).to_bytes(2, "little") + (2048000).to_bytes(4, "little") \
        + (4096000).to_bytes(4, "little") + (2).to_bytes(2, "little") + (8).to_bytes(2, "little")
    body = b"WAVE" + b"fmt " + len(fmt).to_bytes(4, "little") + fmt + b"xtra" + (3).to_bytes(4, "little") + b"abc\0" \
        + b"data" + len(payload).to_bytes(4, "little") + payload
    return b"RIFF" + len(body).to_bytes(4, "little") + body


def _rtl_tcp_server(payload: bytes):
    """One loopback rtl_tcp server (the 12-byte RTL0 dongle_info, then the samples); returns (port, thread)."""
    srv = socket.socket(socket.AF_INET, socket.SOCK_STREAM)
    srv.bind(("127.0.0.1", 0))
    srv.listen(1)
    port = srv.getsockname()[1]

    def serve():
        c, _ = srv.accept()
        c.sendall(b"RTL0" + (5).to_bytes(4, "big") + (29).to_bytes(4, "big") + payload)
        c.shutdown(socket.SHUT_WR)
        c.settimeout(10.0)
        try:
            while c.recv(4096):
                pass
        except OSError:
            pass
        c.close()
        srv.close()
    t = threading.Thread(target=serve, daemon=True)
    t.start()
    return port, t


def _read_all(lib, h, n):
    buf = (C.c_ubyte * n)()
    got = C.c_int()
    assert lib.rtlsdr_read_sync(h, buf, n, C.byref(got)) == 0
    return bytes(buf[:got.value])


def test_a_list_of_five_sources(shim, tmp_path, monkeypatch):
    lib = shim
    rng = np.random.default_rng(31)
    data = [rng.integers(0, 256, size=4096 + 512 * i, dtype=np.uint8).tobytes() for i in range(5)]
    paths = []
    for i in (0, 1, 3):
        p = tmp_path / f"s{i}.bin"
        p.write_bytes(data[i])
        paths.append(str(p))
    wav = tmp_path / "s2.wav"
    wav.write_bytes(_wav(data[2]))
    port, t = _rtl_tcp_server(data[4])
    lst = tmp_path / "sources.txt"
    lst.write_text(f"# five dongles\n{paths[0]}\n\n{paths[1]}\n   # the WAV one\n{wav}\r\n{paths[2]}\n"
                   f"tcp://127.0.0.1:{port}\n\n")
    monkeypatch.delenv("RTLSDR_FILE", raising=False)
    monkeypatch.setenv("RTLSDR_FILE_LIST", str(lst))
    assert lib.rtlsdr_get_device_count() == 5
    for i in range(5):
        assert lib.rtlsdr_get_device_name(i) == b"IQ file (rtlsdr_amd file device)"
        m, p, s = C.create_string_buffer(256), C.create_string_buffer(256), C.create_string_buffer(256)
        assert lib.rtlsdr_get_device_usb_strings(i, m, p, s) == 0
        assert (m.value, p.value, s.value) == (b"rtlsdr_amd", b"rtl_tcp" if i == 4 else b"file", b"%08d" % (i + 1))
    assert lib.rtlsdr_get_device_name(5) == b""
    assert lib.rtlsdr_get_device_usb_strings(5, None, None, None) == -2
    h = C.c_void_p()
    assert lib.rtlsdr_open(C.byref(h), 5) == -1
    for i in range(5):
        h = C.c_void_p()
        assert lib.rtlsdr_open(C.byref(h), i) == 0, i
        assert _read_all(lib, h, 1 << 16) == data[i], i
        assert lib.rtlsdr_close(h) == 0
    t.join(10)


def test_rtlsdr_file_wins_over_the_list(shim, tmp_path, monkeypatch):
    lib = shim
    one, two = tmp_path / "one.bin", tmp_path / "two.bin"
    one.write_bytes(b"\x01" * 1024)
    two.write_bytes(b"\x02" * 1024)
    lst = tmp_path / "l.txt"
    lst.write_text(f"{two}\n{two}\n{two}\n")
    monkeypatch.setenv("RTLSDR_FILE_LIST", str(lst))
    monkeypatch.setenv("RTLSDR_FILE", str(one))
    assert lib.rtlsdr_get_device_count() == 1
    s = C.create_string_buffer(256)
    assert lib.rtlsdr_get_device_usb_strings(0, None, None, s) == 0 and s.value == b"00000001"
    assert lib.rtlsdr_get_device_usb_strings(1, None, None, None) == -2
    h = C.c_void_p()
    assert lib.rtlsdr_open(C.byref(h), 1) == -1
    assert lib.rtlsdr_open(C.byref(h), 0) == 0
    assert _read_all(lib, h, 4096) == b"\x01" * 1024
    lib.rtlsdr_close(h)
    # an empty RTLSDR_FILE counts as unset
    monkeypatch.setenv("RTLSDR_FILE", "")
    assert lib.rtlsdr_get_device_count() == 3


def test_two_devices_read_async_at_once(shim, tmp_path, monkeypatch):
    """Each device has its own file, async state and cancel flag: two rtlsdr_read_async loops on two threads deliver
    their own bytes in order, and cancelling one leaves the other running to the end of its file."""
    lib = shim
    L = 16384
    rng = np.random.default_rng(32)
    a = rng.integers(0, 256, size=L * 40, dtype=np.uint8)
    b = rng.integers(0, 256, size=L * 25 + 1024, dtype=np.uint8)
    pa, pb = tmp_path / "a.bin", tmp_path / "b.bin"
    a.tofile(pa)
    b.tofile(pb)
    lst = tmp_path / "l.txt"
    lst.write_text(f"{pa}\n{pb}\n")
    monkeypatch.delenv("RTLSDR_FILE", raising=False)
    monkeypatch.delenv("RTLSDR_FILE_LOOP", raising=False)
    monkeypatch.setenv("RTLSDR_FILE_LIST", str(lst))
    ha, hb = C.c_void_p(), C.c_void_p()
    assert lib.rtlsdr_open(C.byref(ha), 0) == 0 and lib.rtlsdr_open(C.byref(hb), 1) == 0
    got = {0: [], 1: []}
    stop_a_after = 7
    both_running = threading.Barrier(2, timeout=10)

    def cb_a(buf, n, ctx):
        got[0].append(bytes(C.string_at(buf, n)))
        if len(got[0]) == 1:
            both_running.wait()
        if len(got[0]) == stop_a_after:
            assert lib.rtlsdr_cancel_async(ha) == 0

    def cb_b(buf, n, ctx):
        got[1].append(bytes(C.string_at(buf, n)))
        if len(got[1]) == 1:
            both_running.wait()
    fa, fb = CB(cb_a), CB(cb_b)
    rc = {}
    ta = threading.Thread(target=lambda: rc.__setitem__(0, lib.rtlsdr_read_async(ha, fa, None, 4, L)))
    tb = threading.Thread(target=lambda: rc.__setitem__(1, lib.rtlsdr_read_async(hb, fb, None, 4, L)))
    ta.start()
    tb.start()
    ta.join(30)
    tb.join(30)
    assert rc == {0: 0, 1: 0}
    assert len(got[0]) == stop_a_after and b"".join(got[0]) == a[:L * stop_a_after].tobytes()
    assert len(got[1]) == 26 and b"".join(got[1]) == b.tobytes()
    # a cancelled device reads on from where it stopped
    assert lib.rtlsdr_cancel_async(ha) == -2
    rest = _read_all(lib, ha, L * 40)
    assert rest == a[L * stop_a_after:].tobytes()
    lib.rtlsdr_close(ha)
    lib.rtlsdr_close(hb)


@pytest.mark.parametrize("argv,why", [
    (["-N", "3", "-f", "100M", "out.raw"], "%d"),
    (["-N", "2", "-f", "100M", "-"], "stdout"),
    (["-N", "2", "-f", "1M", "-f", "2M", "-f", "3M", "out_%d.raw"], "-f once"),
    (["-N", "2", "-f", "100M", "-Z", "out_%d.raw"], "-Z"),
    (["-N", "0", "-f", "100M", "out_%d.raw"], "-N"),
])
def test_cli_refuses_what_N_does_not_allow(tmp_path, argv, why):
    """These are usage errors, found before a device is opened or a GPU handle created (no GPU needed)."""
    _, cli = hipbuild.build_host()
    src = tmp_path / "c.bin"
    src.write_bytes(b"\x80" * 16384 * 2)
    lst = tmp_path / "l.txt"
    lst.write_text(f"{src}\n{src}\n{src}\n")
    env = {k: v for k, v in os.environ.items() if k != "RTLSDR_FILE"}
    env["RTLSDR_FILE_LIST"] = str(lst)
    r = subprocess.run([cli] + argv, env=env, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert why in r.stderr and "Use:" in r.stderr, r.stderr
    assert "rtlfm_gpu_create" not in r.stderr and "Tuned to" not in r.stderr and "tuned to" not in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == ["c.bin", "l.txt"]
