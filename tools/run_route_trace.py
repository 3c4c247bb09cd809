"""One step of every route of an rtl_fm run, for a kernel trace (LAB.md I.53, profiles/run_route_trace.txt).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/run_route_trace.py run NAMES.txt
    python tools/run_route_trace.py report DIR NAMES.txt > LIST.txt

`run` takes the first row of tests/fm_route_rows.py for every distinct (route, rest, squelch, -M raw, audio tail, path)
and runs it once on a fresh handle, a launch of k_rotate_90_u8 (rtlfm_gpu_rotate_90_u8, which no run launches) in front
of it and one behind it; the rows' names go to NAMES.txt in that order.  It calls nothing an earlier build of the library
lacks, so RTLFM_HIP_LIB may name one.  `report` cuts the trace at those launches and prints, per row, the kernels in
dispatch order (template arguments kept, parameter lists cut)."""
import csv
import ctypes as C
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
SEPARATOR = "k_rotate_90_u8"


def rows():
    from fm_route_rows import ROWS
    seen, out = set(), []
    for r in ROWS:
        ov = r["ov"]
        key = (r["want"], r["rest"], bool(ov.get("squelch_level") or ov.get("report_levels")), ov.get("mode", 0) == 4,
               bool(ov.get("deemph") or ov.get("rate_out2", -1) > 0 or ov.get("post_downsample", 1) > 1), r["path"], bool(ov.get("dc_block_raw")))
        if r["gpu"] and r["want"] > 0 and key not in seen:
            seen.add(key)
            out.append(r)
    return out


def run(names_path):
    import torch

    import row_geometry as rg
    import test_fm_route_gpu as t
    from fm_route_rows import PLACES, out_stride
    from rtlsdr_amd import capi
    lib = capi.load()
    mark = torch.zeros(64, dtype=torch.uint8, device="cuda")

    def separator():
        torch.cuda.synchronize()
        assert lib.rtlfm_gpu_rotate_90_u8(0, mark.data_ptr(), 16, None) == 0
        torch.cuda.synchronize()

    names = []
    for r in rows():
        with t._open(r, r["path"]) as g:
            L, nb, S = r["L"], r["nb"], g.nstreams
            iq = t._input(2 if r["chan"] else t.STREAMS, L)[:, :nb * L]
            cap = lib.rtlfm_result_cap(C.byref(g.cfg)) * nb
            din = rg.DeviceInput(iq, 0, 0)
            dout = rg.DeviceOutput(S, cap, PLACES[r["place"]][0], out_stride(r, cap))
            separator()
            g.run_device(din.ptr, din.stride, nb, dout.ptr, dout.stride, dout.len.data_ptr())
            g.sync()
            separator()
            names.append(f"{r['name']} last_path={g.last_path}")
    with open(names_path, "w") as f:
        f.write("\n".join(names) + "\n")
    print(f"{len(names)} rows run")


def report(trace_dir, names_path):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert len(files) == 1, files
    recs = list(csv.DictReader(open(files[0])))
    recs.sort(key=lambda d: int(d.get("Dispatch_Id") or d["Start_Timestamp"]))
    kernels = [d["Kernel_Name"].split("(")[0].replace("void ", "") for d in recs]
    segments, cur, inside = [], [], False
    for k in kernels:
        if k.endswith(SEPARATOR) or k == SEPARATOR:
            if inside:
                segments.append(cur)
            cur, inside = [], not inside
        elif inside:
            cur.append(k)
    names = open(names_path).read().split("\n")[:-1]
    assert len(segments) == len(names), (len(segments), len(names))
    for n, seg in zip(names, segments, strict=True):
        print(f"{n}: " + ", ".join(seg))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(sys.argv[2])
    else:
        report(sys.argv[2], sys.argv[3])
