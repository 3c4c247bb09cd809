"""The arithmetic of tests/row_geometry.py, with numpy arrays in the tensors' place: the addresses each named geometry
gives nine rows, and what the guard checker sees."""
import numpy as np
import pytest

import row_geometry as rg

NS = rg.STREAMS
ROW_BYTES = 3 * 16384          # nb * L of the rtl_fm cases
CAPS = [3 * 1026, 3 * 8195, 771, 2 * 98306]   # rtlfm_result_cap() * nblocks of a few configurations: even, odd, small, large
BASES = [0, 256, 4096 + 64, 1 << 21]          # where an allocator may put the allocation (always 64-byte aligned or better)


def out_addrs(name, cap, base):
    g = rg.GEOMETRIES[name]
    return rg.OutputPlan(base, NS, cap, g["out_off"], rg.out_stride(name, cap)).row_addrs()


def in_addrs(name, base):
    g = rg.GEOMETRIES[name]
    return rg.InputPlan(base, NS, ROW_BYTES, g["in_off"], g["in_pad"]).row_addrs()


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("cap", CAPS)
def test_output_addresses_are_what_the_table_claims(cap, base):
    every_piece = set(range(0, 128, 16))
    # line: every row on a 128-byte line
    assert {a % 128 for a in out_addrs("line", cap, base)} == {0}
    # piece: 16-byte aligned, rows walk all eight 16-byte phases of a line, the first 16 bytes behind one, and wrap
    a = out_addrs("piece", cap, base)
    assert [x % 128 for x in a] == [(16 + 16 * k) % 128 for k in range(NS)]
    assert {x % 128 for x in a} == every_piece and {x % 16 for x in a} == {0}
    # dword: 4-byte aligned only; element phases 2, 4, 6, 0 modulo 8, every one at least twice in nine rows
    a = out_addrs("dword", cap, base)
    assert [x % 16 for x in a] == [(4 + 4 * k) % 16 for k in range(NS)]
    assert {x % 16 for x in a} == {0, 4, 8, 12}
    assert all([x % 16 for x in a].count(p) >= 2 for p in (0, 4, 8, 12))
    # dword6: the other rotation, 6, 4, 2, 0
    a = out_addrs("dword6", cap, base)
    assert [x % 16 for x in a] == [(12 + 12 * k) % 16 for k in range(NS)]
    assert {x % 16 for x in a} == {0, 4, 8, 12}
    for name in rg.GEOMETRIES:
        st = rg.out_stride(name, cap)
        g = rg.GEOMETRIES[name]
        assert cap <= st < cap + g["out_mod"] and st % g["out_mod"] == g["out_rem"] and st % 2 == 0, (name, cap, st)
        assert out_addrs(name, cap, base)[0] % 128 == 2 * g["out_off"]


@pytest.mark.parametrize("base", BASES)
def test_input_addresses_are_what_the_table_claims(base):
    every_piece = set(range(0, 128, 16))
    assert {a % 128 for a in in_addrs("line", base)} == {0}
    a = in_addrs("piece", base)
    assert [x % 128 for x in a] == [(16 + 16 * k) % 128 for k in range(NS)] and {x % 128 for x in a} == every_piece
    a = in_addrs("dword", base)
    assert [x % 128 for x in a] == [(48 + 16 * k) % 128 for k in range(NS)] and {x % 128 for x in a} == every_piece
    a = in_addrs("dword6", base)
    assert [x % 128 for x in a] == [(112 + 48 * k) % 128 for k in range(NS)] and {x % 128 for x in a} == every_piece
    for name, g in rg.GEOMETRIES.items():
        p = rg.InputPlan(base, NS, ROW_BYTES, g["in_off"], g["in_pad"])
        assert {x % 16 for x in p.row_addrs()} == {0} and p.stride % 16 == 0 and p.stride == ROW_BYTES + g["in_pad"]
        assert p.total <= rg.InputPlan.room(NS, ROW_BYTES, g["in_off"], g["in_pad"])
        assert p.start >= rg.IN_MARGIN and p.total - (p.start + NS * p.stride) >= rg.IN_MARGIN


@pytest.mark.parametrize("off,pad", [(0, 0), (16, 16), (48, 80), (4, 8), (1, 1), (16, 8)])
def test_input_rows_and_fill_are_where_the_plan_says(off, pad):
    rows = np.arange(3 * 1000, dtype=np.uint32).reshape(3, 1000).astype(np.uint8) | 1   # never 0: the fill is
    buf = np.empty(rg.InputPlan.room(3, 1000, off, pad), dtype=np.uint8)
    p = rg.InputPlan(buf.ctypes.data, 3, 1000, off, pad)
    rg.place_input(buf, p, rows, 0x00)
    assert p.addr % 128 == off and p.addr == buf.ctypes.data + p.start
    for k in range(3):
        a = p.start + k * p.stride
        assert np.array_equal(buf[a:a + 1000], rows[k])
    assert int((buf != 0).sum()) == 3 * 1000
    rg.place_input(buf, p, rows, 0xFF)
    assert int((buf == 0xFF).sum()) >= buf.size - 3 * 1000 and np.array_equal(buf[p.start:p.start + 1000], rows[0])


@pytest.mark.parametrize("name", list(rg.GEOMETRIES))
def test_guard_checker(name):
    g = rg.GEOMETRIES[name]
    cap = 771
    st = rg.out_stride(name, cap)
    arr = np.full(rg.OutputPlan.room(NS, cap, g["out_off"], st), rg.SENTINEL, dtype=np.int16)
    p = rg.OutputPlan(arr.ctypes.data, NS, cap, g["out_off"], st)
    assert p.total <= arr.size and p.start >= rg.OUT_MARGIN and arr.size - (p.start + (NS - 1) * st + cap) >= rg.OUT_MARGIN
    assert rg.stray(arr, p).size == 0
    # nothing inside a window counts: first and last element of every row, and a whole row
    for k in range(NS):
        p.row(arr, k)[0] = 1
        p.row(arr, k)[cap - 1] = 2
    p.row(arr, 4)[:] = 7
    assert rg.stray(arr, p).size == 0
    # one changed element in the front margin, in a gap, in the back margin - the elements next to a window included
    places = {"front margin": [0, p.start - 1], "back margin": [p.start + (NS - 1) * st + cap, arr.size - 1]}
    if st > cap:
        places["gap"] = [p.start + cap, p.start + st - 1, p.start + 5 * st + cap]
    else:
        assert name == "line" and cap % 64 == 0
    for what, idx in places.items():
        for i in idx:
            keep = arr[i]
            arr[i] = 0
            assert rg.stray(arr, p).tolist() == [i], (what, i)
            arr[i] = keep
    assert rg.stray(arr, p).size == 0


def test_guard_checker_sees_the_gap_of_every_named_geometry():
    """cap = 771 leaves a gap in every geometry (the line geometry rounds it up to 832)."""
    for name in rg.GEOMETRIES:
        assert rg.out_stride(name, 771) > 771, name
