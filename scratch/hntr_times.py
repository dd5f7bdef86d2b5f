"""Times Hntr.regrid_device from 1-minute fields (Hntr; profiles/hntr_*.txt): 1' -> 1 deg and 1' -> 1/2 deg at
1 and 8 fields with a shared weight, and 1' -> 4 x 5 deg (the chain-bound case).  Device events around `reps` launches
after a warm-up; the algorithmic bytes are sW*nA*(weight planes) + sS*nvar*nA + 8*nvar*nB.  Run it under rocprofv3
--kernel-trace --stats for kernel times.

  hntr_times.py [reps]                       the double path, as before
  hntr_times.py typed [reps]                 the forms (f64, f64), (const, f64), (const, i16), (i16, i16), alternating inside one run
  hntr_times.py host                         ibh_hntr_regrid_host against ibh_hntr_regrid_typed_host, one 1' field (PCIe dominates)
  hntr_times.py gate PARENT_LIB [reps]       the double path of this library against another build's (the parent commit's
                                             libicebin_hip.so), alternating; the allowed difference is the parent's own spread"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from icebin_amd import Hntr, HntrSpec  # noqa: E402

PEAK = 8e12
CASES = [("1min_to_1deg", (360, 180, 0., 60.), 1), ("1min_to_1deg", (360, 180, 0., 60.), 8),
         ("1min_to_halfdeg", (720, 360, 0., 30.), 1), ("1min_to_halfdeg", (720, 360, 0., 30.), 8),
         ("1min_to_4x5deg", (72, 45, 0., 240.), 1)]
A1MIN = (21600, 10800, 0., 1.)
FORMS = [("f64", "f64"), ("const", "f64"), ("const", "i16"), ("i16", "i16")]
SIZE = {"f64": 8, "i16": 2, "f32": 4, "const": 0}


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def report(**kw):
    print(json.dumps(kw), flush=True)


def main(reps=5):
    dev = torch.device("cuda:0")
    A = HntrSpec(*A1MIN)
    g = torch.Generator(device=dev).manual_seed(1)
    W = torch.rand(A.size, dtype=torch.float64, device=dev, generator=g)
    X = torch.rand((8, A.size), dtype=torch.float64, device=dev, generator=g)
    for name, bdef, nvar in CASES:
        B = HntrSpec(*bdef)
        h = Hntr(17.17, B, A, -1e30)
        out = h.regrid_device(W, X[:nvar])
        torch.cuda.synchronize()
        n = reps if B.size >= 64800 else 2
        ms = timed(lambda: h.regrid_device(W, X[:nvar], out=out), n)
        nbytes = 8 * (nvar + 1) * A.size + 8 * nvar * B.size
        report(case=name, B="%dx%d" % (B.im, B.jm), nvar=nvar, ms=round(ms, 4), GBps=round(nbytes / ms / 1e6, 1),
               share_of_8TBps=round(nbytes / PEAK / (ms * 1e-3), 3), floor_ms=round(nbytes / PEAK * 1e3, 4))
        del h


def typed_inputs(dev, A, nvar):
    g = torch.Generator(device=dev).manual_seed(1)
    X16 = torch.randint(-11000, 8851, (nvar, A.size), dtype=torch.int16, device=dev, generator=g)
    W16 = torch.randint(0, 3, (A.size,), dtype=torch.int16, device=dev, generator=g)
    return {"f64": X16.to(torch.float64), "i16": X16}, {"f64": W16.to(torch.float64), "i16": W16, "const": 1.0}


def typed(reps=5, rounds=3):
    """Every form `rounds` times, the forms alternating; each timing is the mean of `reps` launches."""
    dev = torch.device("cuda:0")
    A = HntrSpec(*A1MIN)
    X, W = typed_inputs(dev, A, 8)
    for name, bdef, nvar in CASES[:4]:
        B = HntrSpec(*bdef)
        h = Hntr(17.17, B, A, -1e30)
        outs, series = {}, {f: [] for f in FORMS}
        for wf, sf in FORMS:        # warm-up; the forms agree bit for bit where their values agree
            outs[(wf, sf)] = h.regrid_device(W[wf], X[sf][:nvar])
        torch.cuda.synchronize()
        assert torch.equal(outs[("const", "f64")], outs[("const", "i16")]) and torch.equal(outs[("f64", "f64")], outs[("i16", "i16")])
        for _ in range(rounds):
            for wf, sf in FORMS:
                series[(wf, sf)].append(timed(lambda: h.regrid_device(W[wf], X[sf][:nvar], out=outs[(wf, sf)]), reps))
        for wf, sf in FORMS:
            ms = min(series[(wf, sf)])
            nbytes = SIZE[wf] * A.size + SIZE[sf] * nvar * A.size + 8 * nvar * B.size
            shape = h.regrid_shape(nvar, None if wf == "const" else W[wf].dtype, X[sf].dtype)
            report(case=name, B="%dx%d" % (B.im, B.jm), nvar=nvar, weight=wf, source=sf, ms=round(ms, 4),
                   ms_all=[round(t, 4) for t in series[(wf, sf)]], bytes=nbytes, share_of_8TBps=round(nbytes / PEAK / (ms * 1e-3), 3),
                   floor_ms=round(nbytes / PEAK * 1e3, 4), **shape)
        del h


def host(reps=2):
    from icebin_amd._capi import check, lib, ptr
    A, B = HntrSpec(*A1MIN), HntrSpec(720, 360, 0., 30.)
    h = Hntr(17.17, B, A, -1e30)
    rng = np.random.default_rng(1)
    X16 = rng.integers(-11000, 8851, A.size).astype(np.int16)
    W16 = rng.integers(0, 3, A.size).astype(np.int16)
    Xd, Wd = X16.astype(np.float64), W16.astype(np.float64)
    out, results = np.empty(B.size), {}

    def run(w, wt, wc, x, at):
        if at is None:
            check(lib().ibh_hntr_regrid_host(h._h, ptr(w), 0, ptr(x), 1, A.size, ptr(out), B.size, 0, 1., 0.))
        else:
            check(lib().ibh_hntr_regrid_typed_host(h._h, None if w is None else ptr(w), wt, 0, wc, ptr(x), at, 1, A.size, ptr(out), B.size,
                                                   0, 1., 0.))

    forms = [("ibh_hntr_regrid_host (f64, f64)", (Wd, 0, 0., Xd, None), 16), ("typed_host (f64, f64)", (Wd, 0, 0., Xd, 0), 16),
             ("typed_host (i16, i16)", (W16, 1, 0., X16, 1), 4), ("typed_host (const, i16)", (None, 0, 1., X16, 1), 2)]
    for name, args, bpc in forms:
        run(*args)      # warm-up: the device buffers come from the cache afterwards
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run(*args)
            ts.append((time.perf_counter() - t0) * 1e3)
        results[name] = out.copy()
        report(host_form=name, ms=round(min(ts), 2), ms_all=[round(t, 2) for t in ts], bytes_in=bpc * A.size,
               GBps_in=round(bpc * A.size / min(ts) / 1e6, 2))
    assert all(np.array_equal(results[forms[0][0]], results[forms[k][0]]) for k in (1, 2)), "the widths disagree"


SIG = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_double, C.c_void_p]


def gate(parent_lib, reps=5, rounds=5):
    """The four (f64, f64) cases through ibh_hntr_regrid_device of both libraries, alternating; per case both series and
    whether this library's best time lies within the parent's own spread (max - min) of the parent's best."""
    from icebin_amd._capi import lib
    dev = torch.device("cuda:0")
    A = HntrSpec(*A1MIN)
    g = torch.Generator(device=dev).manual_seed(1)
    W = torch.rand(A.size, dtype=torch.float64, device=dev, generator=g)
    X = torch.rand((8, A.size), dtype=torch.float64, device=dev, generator=g)
    libs = {"parent": C.CDLL(parent_lib), "this": lib()}
    for L in libs.values():
        L.ibh_hntr_create.restype = C.c_int
        L.ibh_hntr_create.argtypes = [C.POINTER(C.c_void_p)] + [C.c_int32, C.c_int32, C.c_double, C.c_double] * 2 + [C.c_double]
        L.ibh_hntr_regrid_device.restype = C.c_int
        L.ibh_hntr_regrid_device.argtypes = SIG
        L.ibh_hntr_destroy.argtypes = [C.c_void_p]
    s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ok = True
    for name, bdef, nvar in CASES[:4]:
        B = HntrSpec(*bdef)
        hs, outs = {}, {}
        for k, L in libs.items():
            hs[k] = C.c_void_p()
            assert L.ibh_hntr_create(C.byref(hs[k]), A.im, A.jm, A.offi, A.dlat, B.im, B.jm, B.offi, B.dlat, -1e30) == 0
            outs[k] = torch.empty((nvar, B.size), dtype=torch.float64, device=dev)

        def launch(k):
            rc = libs[k].ibh_hntr_regrid_device(hs[k], W.data_ptr(), 0, X.data_ptr(), nvar, A.size, outs[k].data_ptr(), B.size, 0, 1., 0., s)
            assert rc == 0

        for k in libs:
            launch(k)
        torch.cuda.synchronize()
        assert torch.equal(outs["parent"], outs["this"]), "the double path changed its bits"
        series = {k: [] for k in libs}
        for _ in range(rounds):
            for k in libs:
                series[k].append(timed(lambda: launch(k), reps))
        spread = max(series["parent"]) - min(series["parent"])
        within = min(series["this"]) <= min(series["parent"]) + spread
        ok = ok and within
        report(gate=name, B="%dx%d" % (B.im, B.jm), nvar=nvar, parent_ms=[round(t, 4) for t in series["parent"]],
               this_ms=[round(t, 4) for t in series["this"]], parent_spread_ms=round(spread, 4),
               this_best_minus_parent_best_ms=round(min(series["this"]) - min(series["parent"]), 4), within_parent_spread=within)
        for k, L in libs.items():
            L.ibh_hntr_destroy(hs[k])
    report(gate="all", within_parent_spread=ok)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "typed":
        typed(int(sys.argv[2]) if len(sys.argv) > 2 else 5)
    elif mode == "host":
        host()
    elif mode == "gate":
        gate(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    else:
        main(int(mode) if mode else 5)
