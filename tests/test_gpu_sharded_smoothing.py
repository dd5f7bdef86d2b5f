"""Smoothed IvA / IvE on several ranks: the shared smoothed build (ibh_regrid_matrices_matrix_d_sharded_sigma), the sharded
applies with the conservation correction (ibh_weighted_apply_(many_)sharded_conserve_device) and the reproducible member order
of the smoothing's spatial bins that makes a bitwise claim possible.  The ranks are spawned processes sharing the box's one GPU
over a host-staged gloo transport (equal blocks and pieces of unequal size), as in test_distributed_gloo.py."""
import ctypes as C
import math
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIGMA = (50e3, 50e3, 100.0)
TRIPLET, DIRECT, TILE = 1, 2, 3                 # linear_Weighted.smoothed_by()
PAIRS = ((True, True), (True, False), (False, True), (False, False))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _built_code(w):
    from icebin_amd import _capi
    v = C.c_int()
    _capi.check(_capi.lib().ibh_weighted_built_fast(w._h, C.byref(v)))
    return v.value


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_matrix(a, b):
    """dims, CSR, val bits, wM, Mw, conservative"""
    if (a.nrow_d, a.ncol_d, a.nnz, a.conservative) != (b.nrow_d, b.ncol_d, b.nnz, b.conservative):
        return False
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in
               zip(a.csr_dense() + (a.wM, a.Mw, a.dim(0), a.dim(1)), b.csr_dense() + (b.wM, b.Mw, b.dim(0), b.dim(1))))


def _conservation(w, x, y):
    a = math.fsum((w.Mw * x).tolist())
    b = math.fsum((w.wM * y).tolist())
    return abs(a - b) / abs(a)


def _transport(world, rank, stage_mb):
    """a host-staged gloo transport for ibh_comm_create_custom: equal blocks and pieces of unequal size, synchronous on the
    stream the library hands in"""
    rt = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    rt.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    rt.hipStreamSynchronize.argtypes = [C.c_void_p]
    stage = torch.empty(stage_mb << 20, dtype=torch.uint8).pin_memory()
    calls = {"blocks": 0, "gatherv": 0}

    def move(d_base, pieces, r_, stream):
        maxn = max(n for _, n in pieces)
        off, n = pieces[r_]
        assert maxn * (len(pieces) + 1) <= stage.numel()
        mine = stage[:maxn]
        if n:
            assert rt.hipMemcpyAsync(mine.data_ptr(), d_base + off, n, 2, stream) == 0
        assert rt.hipStreamSynchronize(stream) == 0
        parts = [torch.empty(maxn, dtype=torch.uint8) for _ in pieces]
        dist.all_gather(parts, mine.clone())
        for k, (offk, nk) in enumerate(pieces):
            if k != r_ and nk:
                dst = stage[(k + 1) * maxn:(k + 1) * maxn + nk]
                dst.copy_(parts[k][:nk])
                assert rt.hipMemcpyAsync(d_base + offk, dst.data_ptr(), nk, 1, stream) == 0
        assert rt.hipStreamSynchronize(stream) == 0

    def exchange(d_base, count, stride, w_, r_, stream):
        calls["blocks"] += 1
        move(d_base, [(8 * k * stride, 8 * count) for k in range(w_)], r_, stream)

    def gatherv(d_base, offs, w_, r_, stream):
        calls["gatherv"] += 1
        move(d_base, [(offs[k], offs[k + 1] - offs[k]) for k in range(w_)], r_, stream)

    return exchange, gatherv, calls


def _worker(rank, world, port, q, job, args):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from icebin_amd.distributed import Communicator
        torch.cuda.set_device(0)                        # the ranks share the box's one card: the transport is host-staged
        exchange, gatherv, calls = _transport(world, rank, 256)
        comm = Communicator(world, rank, exchange=exchange, gatherv=gatherv)
        ok, notes = JOBS[job](comm, world, rank, *args)
        q.put((rank, ok, notes, dict(calls)))
        torch.cuda.synchronize()
        comm.close()
    finally:
        dist.destroy_process_group()


def _spawn(world, job, args=(), timeout=600):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, job, args)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout)
        assert p.exitcode == 0
    return sorted(q.get(timeout=5) for _ in range(world))


# ---- the shared smoothed build ---------------------------------------------------------------------------------------------
FORMS = {                                       # (smooth_direct, smooth_tile) and the built_fast code the form gives
    "size": (-1, -1),                           # by size: spatial tiles at 5 km (shared), the direct form at 20 km
    "tile": (0, 1),
    "direct": (1, 0),
    "triplet": (0, 0),
}


def _job_build(comm, world, rank, cases):
    """cases: (config, knobs of FORMS, sigma, {matrix: (built_fast code, smoothed_by form)}) -- per matrix: at one sigma the tiles may
    serve IvA (shared) and overflow for IvE (every rank steps down to a redundant build)"""
    import icebin_amd
    from icebin_amd import synthetic as syn
    from icebin_amd.linear import set_tuning
    ok, notes = True, []
    for config, form, sigma, expects in cases:
        g = syn.make_grids(config)
        em = syn.dome_elevmask(g)
        mm = icebin_amd.from_synthetic(g)
        rm = mm.regrid_matrices("greenland", em)
        direct, tile = FORMS[form]
        set_tuning("smooth_direct", direct)
        set_tuning("smooth_tile", tile)
        try:
            jobs = [(name, s, c) for name in ("IvA", "IvE") for s, c in PAIRS]
            for name, scale, correctA in jobs:
                ws = rm.matrix_d_sharded(comm, name, scale=scale, correctA=correctA, sigma=sigma)
                w1 = rm.matrix_d(name, scale=scale, correctA=correctA, sigma=sigma)
                good = _same_matrix(ws, w1) and not ws.conservative and (_built_code(ws), ws.smoothed_by()) == expects[name] and \
                    w1.smoothed_by() == expects[name][1]
                if not good:
                    notes.append("%s %s %s scale=%d correctA=%d: built %d by form %d (one rank: form %d)" %
                                 (config, form, name, scale, correctA, _built_code(ws), ws.smoothed_by(), w1.smoothed_by()))
                ok = ok and good
            # the coupler's call (IceCoupler.cpp:461-467): IvE on the identity dimI and the dimE an earlier EvI numbered
            nE = g["nA"] * len(g["hcdefs"])
            got = []
            for sharded in (True, False):
                dimI, dimE = icebin_amd.SparseSet.identity(g["nI"]), icebin_amd.SparseSet(nE)
                build = (lambda n, d, **kw: rm.matrix_d_sharded(comm, n, d, **kw)) if sharded else (lambda n, d, **kw: rm.matrix_d(n, d, **kw))
                build("EvI", (dimE, dimI), scale=False, correctA=False)
                got.append(build("IvE", (dimI, dimE), scale=True, correctA=True, sigma=sigma))
            good = _same_matrix(got[0], got[1]) and (_built_code(got[0]), got[0].smoothed_by()) == expects["IvE"] and \
                got[1].smoothed_by() == expects["IvE"][1]
            if not good:
                notes.append("%s %s coupler IvE: built %d by form %d" % (config, form, _built_code(got[0]), got[0].smoothed_by()))
            ok = ok and good
        finally:
            set_tuning("smooth_direct", -1)
            set_tuning("smooth_tile", -1)
    return ok, notes


def _job_refusals(comm, world, rank):
    import icebin_amd
    from icebin_amd import _capi, synthetic as syn
    ok, notes = True, []
    g = syn.make_grids("g20")
    em = syn.dome_elevmask(g)
    rm = icebin_amd.from_synthetic(g).regrid_matrices("greenland", em)
    for name, sigma, code in (("XvE", SIGMA, _capi.IBH_ENOTIMPL), ("XvA", SIGMA, _capi.IBH_ENOTIMPL),
                              ("IvA", (50e3, 0.0, 100.0), _capi.IBH_EINVAL), ("IvE", (50e3, 50e3, -1.0), _capi.IBH_EINVAL)):
        try:
            rm.matrix_d_sharded(comm, name, sigma=sigma)
            ok = False
            notes.append("%s %s: no error" % (name, sigma))
        except _capi.IcebinHipError as e:
            if e.code != code:
                notes.append("%s %s: code %d" % (name, sigma, e.code))
            ok = ok and e.code == code
    # zero sigma: the unsmoothed shared build, bitwise the existing entry and the single-rank build
    for name in ("IvA", "IvE", "AvI"):
        ws = rm.matrix_d_sharded(comm, name, scale=True, correctA=True, sigma=(0.0, 0.0, 0.0))
        h = C.c_void_p()
        _capi.check(_capi.lib().ibh_regrid_matrices_matrix_d_sharded(rm._h, comm._h, name.encode(), None, None, 1, 1, C.byref(h)))
        from icebin_amd.linear import linear_Weighted
        wo = linear_Weighted(h, keep=(rm,))
        w1 = rm.matrix_d(name, scale=True, correctA=True)
        good = _same_matrix(ws, wo) and _same_matrix(ws, w1) and ws.conservative and _built_code(ws) == 3
        if not good:
            notes.append("%s zero sigma" % name)
        ok = ok and good
    return ok, notes


# ---- the conserving sharded applies ----------------------------------------------------------------------------------------
def _job_apply(comm, world, rank, configs):
    import icebin_amd
    from icebin_amd import _capi, synthetic as syn
    from icebin_amd.distributed import FieldShardedApply, apply_many_sharded, apply_sharded
    from oracle import oracle as orc
    ok, notes = True, []

    def check(cond, what):
        nonlocal ok
        if not cond:
            notes.append(what)
        ok = ok and bool(cond)

    for config in configs:
        g = syn.make_grids(config)
        em = syn.dome_elevmask(g)
        rm = icebin_amd.from_synthetic(g).regrid_matrices("greenland", em, scale=True, correctA=True)
        w = rm.matrix_d("IvE", scale=True, correctA=True, sigma=SIGMA)
        check(not w.conservative, config + " conservative")
        o = orc.Regridder(g).matrix_d("IvE", em, scale=True, correctA=True, sigma=SIGMA) if config == "g20" else None
        nl = 6
        x_all = syn.fields(world * nl, w.ncol_d, seed=17) + 2.0          # the same on every rank
        ld = (w.nrow_d + 63) // 64 * 64
        x_loc = torch.from_numpy(x_all[rank * nl:(rank + 1) * nl].copy()).cuda()

        def ref_rows(p, bf, fc=True):
            xp = torch.from_numpy(x_all[p * nl:(p + 1) * nl].copy()).cuda()
            bf = bf or nl
            return np.concatenate([w.apply_device(xp[f0:f0 + bf].contiguous(), fill=-2.0, force_conservation=fc).cpu().numpy()
                                   for f0 in range(0, nl, bf)])

        for bf in (0, 4, 2):
            out = torch.full((world * nl, ld), -9.0, dtype=torch.float64, device="cuda")[:, : w.nrow_d]
            apply_sharded(w, comm, x_loc, out_all=out, fill=-2.0, block_fields=bf, force_conservation=True)
            comm.wait()
            torch.cuda.synchronize()
            y = out.cpu().numpy()
            for p in range(world):
                check(np.array_equal(_bits(y[p * nl:(p + 1) * nl]), _bits(ref_rows(p, bf))), "%s bf=%d rank %d rows" % (config, bf, p))
            for k in range(world * nl):
                c = _conservation(w, x_all[k], y[k])
                check(c < 1e-13, "%s bf=%d field %d conservation %.3g" % (config, bf, k, c))
            if o is not None:
                ref = o.apply(x_all, fill=-2.0, force_conservation=True)
                err = np.max(np.abs(y - ref)) / np.max(np.abs(ref))
                check(err <= 1e-12, "%s bf=%d oracle %.3g" % (config, bf, err))
            # force_conservation = 0: the existing entry, bitwise
            out0 = torch.full((world * nl, ld), -9.0, dtype=torch.float64, device="cuda")[:, : w.nrow_d]
            outx = torch.full((world * nl, ld), -9.0, dtype=torch.float64, device="cuda")[:, : w.nrow_d]
            apply_sharded(w, comm, x_loc, out_all=out0, fill=-2.0, block_fields=bf, force_conservation=False)
            s = torch.cuda.current_stream().cuda_stream
            _capi.check(_capi.lib().ibh_weighted_apply_sharded_device(w._h, comm._h, C.c_void_p(x_loc.data_ptr()), nl, w.ncol_d,
                                                                      C.c_void_p(outx.data_ptr()), ld, -2.0, bf, C.c_void_p(s)))
            comm.wait()
            torch.cuda.synchronize()
            check(np.array_equal(_bits(out0.cpu().numpy()), _bits(outx.cpu().numpy())), "%s bf=%d uncorrected" % (config, bf))
            check(not np.array_equal(_bits(out0.cpu().numpy()), _bits(y)), "%s bf=%d the correction changed nothing" % (config, bf))
        # the result as a column view of a wider array: nothing outside the view changes on any rank
        left, right = 5, 7
        wide = torch.full((world * nl, w.nrow_d + left + right), float(rank + 7), dtype=torch.float64, device="cuda")
        apply_sharded(w, comm, x_loc, out_all=wide[:, left:left + w.nrow_d], fill=-2.0, force_conservation=True)
        comm.wait()
        torch.cuda.synchronize()
        hw = wide.cpu().numpy()
        check(np.all(hw[:, :left] == rank + 7) and np.all(hw[:, left + w.nrow_d:] == rank + 7), config + " view: outside touched")
        for p in range(world):
            check(np.array_equal(_bits(hw[p * nl:(p + 1) * nl, left:left + w.nrow_d]), _bits(ref_rows(p, 0))), "%s view rank %d" % (config, p))
        # three batches: one SpMM launch, one grouped exchange, each batch corrected
        nb = 3
        xb = [syn.fields(world * nl, w.ncol_d, seed=31 + k) + 1.0 for k in range(nb)]
        big = torch.full((nb, world * nl, ld), -9.0, dtype=torch.float64, device="cuda")
        xs = [torch.from_numpy(xa[rank * nl:(rank + 1) * nl].copy()).cuda() for xa in xb]
        apply_many_sharded(w, comm, xs, [big[k][:, : w.nrow_d] for k in range(nb)], fill=-2.0, force_conservation=True)
        comm.wait()
        torch.cuda.synchronize()
        hb = big[:, :, : w.nrow_d].cpu().numpy()
        for k in range(nb):
            for p in range(world):
                xp = torch.from_numpy(xb[k][p * nl:(p + 1) * nl].copy()).cuda()
                ref = w.apply_device(xp, fill=-2.0, force_conservation=True).cpu().numpy()
                check(np.array_equal(_bits(hb[k, p * nl:(p + 1) * nl]), _bits(ref)), "%s many batch %d rank %d" % (config, k, p))
            for f in range(world * nl):
                check(_conservation(w, xb[k][f], hb[k, f]) < 1e-13, "%s many batch %d field %d conservation" % (config, k, f))
        # FieldShardedApply: its local applies (the C-ABI device apply) correct the fields
        sh = FieldShardedApply(w, world * nl, group=None, device=torch.device("cuda", 0), force_conservation=True)
        y = torch.full((nl, ld), -9.0, dtype=torch.float64, device="cuda")
        sh._apply(x_loc.data_ptr(), w.ncol_d, y, -2.0, torch.cuda.current_stream().cuda_stream)
        ys = [torch.full((nl, ld), -9.0, dtype=torch.float64, device="cuda") for _ in range(2)]
        sh._apply_many([x_loc.data_ptr(), xs[0].data_ptr()], w.ncol_d, ys, -2.0, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        check(np.array_equal(_bits(y[:, : w.nrow_d].cpu().numpy()), _bits(ref_rows(rank, 0))), config + " FieldShardedApply")
        ref1 = w.apply_device(xs[0], fill=-2.0, force_conservation=True).cpu().numpy()
        check(np.array_equal(_bits(ys[0][:, : w.nrow_d].cpu().numpy()), _bits(ref_rows(rank, 0))) and
              np.array_equal(_bits(ys[1][:, : w.nrow_d].cpu().numpy()), _bits(ref1)), config + " FieldShardedApply many")
    return ok, notes


JOBS = {"build": _job_build, "refusals": _job_refusals, "apply": _job_apply}


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3])
def test_shared_smoothed_build_is_the_single_rank_build_bitwise(world):
    """5 km, sigma = (50 km, 50 km, 100 m): the spatial-tile form by size, shared by the ranks (built_fast 3) -- IvA and IvE with
    all four (scale, correctA) pairs and the coupler's IvE on the identity dimI and a dimE numbered by an EvI: every rank's matrix
    is bitwise matrix_d(..., sigma) on one rank (dims, CSR, val bits, wM, Mw, conservative = 0); the rows travelled (gatherv)."""
    got = _spawn(world, "build", ([("g5", "size", SIGMA, {"IvA": (3, TILE), "IvE": (3, TILE)})],))
    assert all(ok for _, ok, _, _ in got), got
    assert all(c["gatherv"] > 0 for _, _, _, c in got), got


@pytest.mark.gpu
def test_smoothed_build_forms_on_two_ranks():
    """20 km: the direct form by size and the triplet pipeline (smooth_tile = smooth_direct = 0) run on every rank (built_fast 1),
    the tile form forced (smooth_tile = 1) is shared (3); every result bitwise the single-rank build.  50 km, sigma = (120 km,
    120 km, 400 m), smooth_tile = 1: the tiles serve IvA (45 columns around the widest bin) shared, while IvE (365 > SMT_KMAX) makes
    both ranks step down together to the redundant triplet build (built_fast 1).  Which side of the limits each input lies on is
    asserted here, on the CPU, before any rank starts."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    try:
        import smoothing_cases as smc
    finally:
        sys.path.pop(0)
    sigma_wide = (120e3, 120e3, 400.0)
    cases = [("g20", "size", SIGMA, {"IvA": (1, DIRECT), "IvE": (1, DIRECT)}), ("g20", "triplet", SIGMA, {"IvA": (1, TRIPLET), "IvE": (1, TRIPLET)}),
             ("g20", "tile", SIGMA, {"IvA": (3, TILE), "IvE": (3, TILE)}), ("g50", "tile", sigma_wide, {"IvA": (3, TILE), "IvE": (1, TRIPLET)})]
    for config, form, sigma, expects in cases:
        direct, tile = FORMS[form]
        for name, (_, by) in expects.items():
            _, _, widest, longest, longest_smoothed = smc.oracle_case(config, name, sigma)
            # ("size": 20 km lies below smooth_direct_max_rows, the direct form is tried and the tiles are not)
            smc.assert_input_side(by, tile > 0, direct > 0 or form == "size", widest, longest, longest_smoothed)
    got = _spawn(2, "build", (cases,))
    assert all(ok for _, ok, _, _ in got), got


@pytest.mark.gpu
def test_shared_smoothed_build_refusals_and_zero_sigma():
    """X-row matrices with sigma != 0: IBH_ENOTIMPL on every rank; a sigma component <= 0: IBH_EINVAL; zero sigma: bitwise the
    existing sharded entry (and the single-rank build), shared."""
    got = _spawn(2, "refusals")
    assert all(ok for _, ok, _, _ in got), got


@pytest.mark.gpu
def test_conserving_sharded_apply_two_ranks():
    """The smoothed IvE (20 km: direct form, 5 km: tiles), 6 fields per rank, field blocks 0 / 4 / 2, force_conservation = 1:
    every rank's rows bitwise that rank's apply_device(force_conservation=True), every field conserved to 1e-13, within 1e-12 of
    the oracle at 20 km; force_conservation = 0 bitwise the existing entry; a column view of a wider array; three batches through
    apply_many_sharded; FieldShardedApply(force_conservation=True)."""
    got = _spawn(2, "apply", (("g20", "g5"),))
    assert all(ok for _, ok, _, _ in got), got


# ---- one rank: the member order of the smoothing's bins does not depend on atomics -----------------------------------------
@pytest.mark.gpu
def test_smoothed_builds_are_reproducible():
    import icebin_amd
    from icebin_amd import synthetic as syn
    from icebin_amd.linear import set_tuning
    from oracle import oracle as orc
    g = syn.make_grids("g5")
    em = syn.dome_elevmask(g)
    rm = icebin_amd.from_synthetic(g).regrid_matrices("greenland", em)
    first = rm.matrix_d("IvE", scale=True, correctA=True, sigma=SIGMA)
    for _ in range(2):
        assert _same_matrix(rm.matrix_d("IvE", scale=True, correctA=True, sigma=SIGMA), first)
    g = syn.make_grids("g20")
    em = syn.dome_elevmask(g)
    rm = icebin_amd.from_synthetic(g).regrid_matrices("greenland", em)
    set_tuning("smooth_direct", 1)
    try:
        ws = [rm.matrix_d("IvA", scale=True, correctA=True, sigma=SIGMA) for _ in range(3)]
    finally:
        set_tuning("smooth_direct", -1)
    assert _same_matrix(ws[1], ws[0]) and _same_matrix(ws[2], ws[0])
    o = orc.Regridder(g).matrix_d("IvA", em, scale=True, correctA=True, sigma=SIGMA)
    row, col, val = ws[0].coo_dense()
    np.testing.assert_array_equal(row, o.row)
    np.testing.assert_array_equal(col, o.col)
    np.testing.assert_allclose(val, o.val, rtol=1e-12, atol=0)
