"""The tool and the device layer around the soft AGC, without a GPU: the gain-index extension symbols of
librtlsdr_file.so, what a tcp:// source sends for gain mode 2 and for an index, and rtl_fm_hip's -O parsing."""
import ctypes as C
import os
import socket
import struct
import subprocess
import threading

import numpy as np
import pytest

from rtlsdr_amd import build as hipbuild


@pytest.fixture(scope="module")
def shim():
    return C.CDLL(hipbuild.build_shim())


def open_dev(shim, monkeypatch, source):
    monkeypatch.setenv("RTLSDR_FILE", str(source))
    shim.rtlsdr_open.argtypes = [C.POINTER(C.c_void_p), C.c_uint32]
    for f in (shim.rtlsdr_close, shim.rtlamd_file_get_gain_index):
        f.argtypes = [C.c_void_p]
    shim.rtlamd_file_set_gain_index.argtypes = [C.c_void_p, C.c_int]
    shim.rtlsdr_set_tuner_gain_mode.argtypes = [C.c_void_p, C.c_int]
    shim.rtlsdr_get_tuner_gains.argtypes = [C.c_void_p, C.c_void_p]
    h = C.c_void_p()
    assert shim.rtlsdr_open(C.byref(h), 0) == 0
    return h


def test_extension_symbols_under_the_rtlamd_prefix(shim):
    out = subprocess.check_output(["nm", "-D", "--defined-only", hipbuild.build_shim()], text=True)
    names = [ln.split()[-1] for ln in out.splitlines() if " T " in ln]
    assert {"rtlamd_file_set_gain_index", "rtlamd_file_get_gain_index", "rtlamd_file_set_buffer_source"} <= set(names)
    assert not [n for n in names if "gain_index" in n and not n.startswith("rtlamd_file_")]
    assert len([n for n in names if n.startswith("rtlsdr_")]) == 26


def test_file_source_records_the_index(shim, monkeypatch, tmp_path):
    p = tmp_path / "in.bin"
    np.zeros(1024, dtype=np.uint8).tofile(p)
    h = open_dev(shim, monkeypatch, p)
    n = shim.rtlsdr_get_tuner_gains(h, None)
    assert n > 1 and shim.rtlamd_file_get_gain_index(h) == 0
    assert shim.rtlamd_file_set_gain_index(h, n - 1) == 0 and shim.rtlamd_file_get_gain_index(h) == n - 1
    assert shim.rtlamd_file_set_gain_index(h, n) == -22 and shim.rtlamd_file_set_gain_index(h, -1) == -22
    assert shim.rtlamd_file_get_gain_index(h) == n - 1
    assert shim.rtlsdr_set_tuner_gain_mode(h, 2) == 0 and shim.rtlamd_file_get_gain_index(h) == 0  # mode 2 starts at 0
    assert shim.rtlamd_file_set_gain_index(None, 0) == -1 and shim.rtlamd_file_get_gain_index(None) == -1
    shim.rtlsdr_close(h)


def test_tcp_source_drives_the_index_in_mode_1(shim, monkeypatch):
    """Gain mode 2 on a tcp:// source asks the server for mode 1 once (it honours index commands in no other) and never
    for its own soft AGC; every index goes out as command 0x0d."""
    srv = socket.socket()
    srv.bind(("127.0.0.1", 0))
    srv.listen(1)
    srv.settimeout(20)  # nothing here may wait for ever: a device layer without the extension never connects
    got = []

    def serve():
        try:
            c, _ = srv.accept()
        except OSError:
            return
        c.settimeout(20)
        try:
            c.sendall(b"RTL0" + struct.pack(">II", 5, 29))
            buf = b""
            while len(buf) < 25:
                d = c.recv(64)
                if not d:
                    break
                buf += d
            got.extend(struct.unpack(">BI", buf[i:i + 5]) for i in range(0, len(buf) - 4, 5))
        except OSError:
            pass
        finally:
            c.close()

    t = threading.Thread(target=serve, daemon=True)
    t.start()
    h = None
    try:
        h = open_dev(shim, monkeypatch, f"tcp://127.0.0.1:{srv.getsockname()[1]}")
        assert shim.rtlsdr_set_tuner_gain_mode(h, 2) == 0
        assert shim.rtlamd_file_set_gain_index(h, 3) == 0
        assert shim.rtlamd_file_set_gain_index(h, 2) == 0
        assert shim.rtlsdr_set_tuner_gain_mode(h, 0) == 0
    finally:
        if h is not None:
            shim.rtlsdr_close(h)  # closes the socket: the server's recv ends
        srv.close()
        t.join(30)
    assert got == [(0x03, 1), (0x0d, 0), (0x0d, 3), (0x0d, 2), (0x03, 0)]


def cli(argv, env_extra):
    _, exe = hipbuild.build_host()
    env = {k: v for k, v in os.environ.items() if k not in ("RTLSDR_FILE", "RTLSDR_FILE_LIST")}
    env.update(env_extra)
    return subprocess.run([exe] + argv, env=env, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("opts", ["agc=7", "agc=", "bw=1500:agc=3", "agc=2:agc=x", "agc=22"])
def test_bad_agc_is_refused_before_a_device_is_opened(opts, tmp_path):
    # the source does not exist: opening it would say "Failed to open rtlsdr device"
    r = cli(["-f", "100M", "-O", opts, str(tmp_path / "out.raw")], {"RTLSDR_FILE": str(tmp_path / "missing.bin")})
    assert r.returncode == 1 and "agc= takes 0" in r.stderr and "Failed to open" not in r.stderr
    assert not (tmp_path / "out.raw").exists()
    r = cli(["-f", "100M", "-N", "2", "-O", opts, str(tmp_path / "out_%d.raw")], {"RTLSDR_FILE_LIST": str(tmp_path / "missing.txt")})
    assert r.returncode == 1 and "agc= takes 0" in r.stderr and "No supported devices" not in r.stderr


@pytest.mark.parametrize("opts", ["bw=1500", "agc=1", "agc=2"])
def test_good_strings_get_as_far_as_the_device(opts, tmp_path):
    r = cli(["-f", "100M", "-O", opts, str(tmp_path / "out.raw")], {"RTLSDR_FILE": str(tmp_path / "missing.bin")})
    assert r.returncode == 1 and "agc= takes" not in r.stderr and "Failed to open rtlsdr device" in r.stderr
