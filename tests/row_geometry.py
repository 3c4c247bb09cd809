"""Device rows at a controlled placement (tests/test_row_geometry_gpu.py, tests/test_power_geometry_gpu.py).  A plain
module, like cases.py.

The C ABI accepts input rows on any 16-byte boundary (rtl_power: anywhere) and output rows on any 4-byte boundary, and
promises the same samples for all of them.  Here the rows of a call lie inside one larger allocation at a chosen offset
from a 128-byte line and a chosen stride; what is not a row is filled - the input's with a byte of the caller's choice,
the output's with a sentinel that `stray` looks for afterwards.

The arithmetic (`InputPlan`, `OutputPlan`, `place_input`, `stray`) works on numpy arrays and plain integers, so that
tests/test_row_geometry_cpu.py checks it without a GPU; `DeviceInput` / `DeviceOutput` put it on torch tensors."""
import numpy as np

LINE = 128            # bytes
IN_MARGIN = 256       # bytes in front of the first input row and behind the last (a multiple of LINE)
OUT_MARGIN = 128      # int16 elements in front of the first output row and behind the last (a multiple of 64)
SENTINEL = -21931     # 0xAA55: what an output allocation holds before the call
STREAMS = 9           # the fewest rows that visit all eight 16-byte phases of a line once and wrap

# name -> output (base_off in int16 elements from a line, stride = cap rounded up to rem modulo mod),
#         input (base_off in bytes from a line, pad in bytes behind every row's payload)
GEOMETRIES = {
    "line":   dict(out_off=0, out_mod=64, out_rem=0, in_off=0, in_pad=0),      # what run_torch() hands over
    "piece":  dict(out_off=8, out_mod=64, out_rem=8, in_off=16, in_pad=16),    # 16-byte aligned, all eight phases of a line
    "dword":  dict(out_off=2, out_mod=8, out_rem=2, in_off=48, in_pad=16),     # 4-byte aligned: element phases 2, 4, 6, 0
    "dword6": dict(out_off=6, out_mod=8, out_rem=6, in_off=112, in_pad=48),    # the other rotation: 6, 4, 2, 0
}


def out_stride(name, cap):
    """The smallest stride >= cap (int16 elements) of the named geometry."""
    g = GEOMETRIES[name]
    return cap + (g["out_rem"] - cap) % g["out_mod"]


class InputPlan:
    """`nrows` rows of `row_bytes` payload bytes, the first `base_off` bytes behind a line, `row_bytes + pad` apart, in an
    allocation that starts at address `base_addr`: `start` (byte index of row 0), `stride`, `total` (bytes needed)."""

    def __init__(self, base_addr, nrows, row_bytes, base_off, pad):
        assert 0 <= base_off < LINE and pad >= 0
        self.nrows, self.row_bytes = nrows, row_bytes
        self.stride = row_bytes + pad
        self.start = (-base_addr) % LINE + IN_MARGIN + base_off
        self.total = self.start + nrows * self.stride + IN_MARGIN
        self.addr = base_addr + self.start

    @staticmethod
    def room(nrows, row_bytes, base_off, pad):
        """Bytes that hold the plan wherever the allocation starts."""
        return LINE - 1 + IN_MARGIN + base_off + nrows * (row_bytes + pad) + IN_MARGIN

    def row_addrs(self):
        return [self.addr + k * self.stride for k in range(self.nrows)]


def place_input(buf, plan, rows, fill):
    """Fill the uint8 array `buf` with `fill` and put rows[k] at the plan's place."""
    assert buf.dtype == np.uint8 and buf.size >= plan.total and rows.shape == (plan.nrows, plan.row_bytes)
    buf[:] = fill
    for k in range(plan.nrows):
        a = plan.start + k * plan.stride
        buf[a:a + plan.row_bytes] = rows[k]


class OutputPlan:
    """`nrows` windows of `cap` int16 elements, the first `base_off` elements behind a line, `st` apart."""

    def __init__(self, base_addr, nrows, cap, base_off, st):
        assert base_addr % 2 == 0 and 0 <= base_off < LINE // 2 and st >= cap
        self.nrows, self.cap, self.stride = nrows, cap, st
        self.start = ((-base_addr) % LINE) // 2 + OUT_MARGIN + base_off
        self.total = self.start + (nrows - 1) * st + cap + OUT_MARGIN
        self.addr = base_addr + 2 * self.start

    @staticmethod
    def room(nrows, cap, base_off, st):
        return LINE // 2 + OUT_MARGIN + base_off + (nrows - 1) * st + cap + OUT_MARGIN

    def row_addrs(self):
        return [self.addr + 2 * k * self.stride for k in range(self.nrows)]

    def row(self, arr, k, n=None):
        a = self.start + k * self.stride
        return arr[a:a + (self.cap if n is None else n)]


def stray(arr, plan, sentinel=SENTINEL):
    """Indices of the elements of `arr` outside every row's window [row_start, row_start + cap) that no longer hold the
    sentinel."""
    changed = arr != sentinel
    for k in range(plan.nrows):
        a = plan.start + k * plan.stride
        changed[a:a + plan.cap] = False
    return np.flatnonzero(changed)


def describe_stray(idx, plan):
    """Where the first few stray elements lie: (row they follow or -1 for the front margin, offset from that row's start)."""
    out = []
    for i in idx[:6].tolist():
        k = min(max((i - plan.start) // plan.stride, -1), plan.nrows - 1)
        out.append((k, i - (plan.start + max(k, 0) * plan.stride)))
    return out


# ------------------------------------------------------------------ on the device ----

class DeviceInput:
    """uint8 rows [nrows, row_bytes] on the device at (base_off, pad); everything else holds `fill`.  `ptr`, `stride`."""

    def __init__(self, rows, base_off, pad, fill=0x00):
        import torch
        self.rows = np.ascontiguousarray(rows, dtype=np.uint8)
        n, nbytes = self.rows.shape
        self.t = torch.empty(InputPlan.room(n, nbytes, base_off, pad), dtype=torch.uint8, device="cuda")
        self.plan = InputPlan(self.t.data_ptr(), n, nbytes, base_off, pad)
        self.ptr, self.stride = self.plan.addr, self.plan.stride
        self.refill(fill)

    def refill(self, fill):
        """The same rows at the same address, the rest filled with another byte."""
        import torch
        host = np.empty(self.t.numel(), dtype=np.uint8)
        place_input(host, self.plan, self.rows, fill)
        self.t.copy_(torch.from_numpy(host))
        torch.cuda.synchronize()


class DeviceOutput:
    """int16 windows of `cap` elements on the device at (base_off, st) in an allocation full of the sentinel."""

    def __init__(self, nrows, cap, base_off, st):
        import torch
        self.t = torch.full((OutputPlan.room(nrows, cap, base_off, st),), SENTINEL, dtype=torch.int16, device="cuda")
        self.plan = OutputPlan(self.t.data_ptr(), nrows, cap, base_off, st)
        self.ptr, self.stride = self.plan.addr, self.plan.stride
        self.len = torch.zeros(nrows, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def read(self):
        """(rows cut to their lengths, lengths, stray indices) once the work is done."""
        host = self.t.cpu().numpy()
        lens = self.len.cpu().numpy()
        assert int(lens.max(initial=0)) <= self.plan.cap and int(lens.min(initial=0)) >= 0, (lens.tolist(), self.plan.cap)
        rows = [self.plan.row(host, k, int(lens[k])).copy() for k in range(self.plan.nrows)]
        return rows, lens, stray(host, self.plan)
