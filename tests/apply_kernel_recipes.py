"""One recipe per apply-kernel instantiation of icebin_amd/csrc/spmm.hip (listed in apply_plan.h): how to make an apply launch exactly that kernel.

A plain module (no tests, no fixtures): tests/test_capi_symbols.py checks that the names below are exactly the apply kernels the
code object holds, tests/test_gpu_apply_kernels.py runs every recipe on the GPU against an exact row-by-row reference.

Each recipe is a dict:
  name     the instantiation as `ibh_weighted_last_launch` (and the demangled code object) spells it;
  family   the matrix: "synthetic" (hand-built CSR through linear_Weighted.from_csr: row lengths around the instantiation's own
           batch sizes, rows of one magnitude with mixed signs, magnitudes spread over 10^+-100), "banded" (hand-built, columns
           of one or two entries in neighbouring rows: a column sweep takes it) or an E-row matrix of the regridder (EvI of a synthetic grid, see
           FAMILIES) whose structures -- bands, row groups, tiles, the column sweep -- the kernel needs;
  kernel   the ibh_weighted_set_kernel request;
  options  per-handle options (ibh_weighted_set_option), never the process-wide map;
  prepare  True: ibh_weighted_prepare builds the structure before the first apply (for "pair": pair_prepare with AvE);
  fb       fields per workgroup (the field chunk of one (row, chunk) task);
  nvars    field counts the layout checks run (every one must launch this instantiation);
  nbatch   batch counts of apply_many_device (empty: the entry takes one batch), each with batch_nvar fields;
  entry    "apply_device", "apply_many_device" or "apply_pair_device".
"""

# the E-row matrices: (grid config, make_grids keywords, spacing of the elevation classes in m or None for the default)
FAMILIES = {
    "g20": ("g20", {}, None),
    "g20_fine": ("g20", dict(nhc=64), 60.0),          # GCM cells with 17..32 classes: the NS = 32 tiles
    "g20_coarse": ("g20", dict(nhc=12), 400.0),       # few classes per cell: the class tables of a fused pair fit 64 KB of LDS
    "g5": ("g5", {}, None),
    "g5_xfast": ("g5", dict(x_fastest=True), None),
}


def _nvars(fb, extra=()):
    """1, FB - 1, FB, FB + 1; 8 chunks (an XCD owns whole chunks) and 3 chunks (contiguous ranges per XCD)."""
    return sorted({1, max(1, fb - 1), fb, fb + 1, 8 * fb, 3 * fb} | set(extra))


def _rowblock():
    out = []
    shapes = [(1, 1, 4), (1, 1, 8), (1, 2, 4), (1, 4, 4), (2, 1, 4), (2, 1, 8), (2, 2, 4), (2, 4, 4),
              (4, 1, 4), (4, 1, 8), (4, 2, 4), (4, 4, 4), (8, 1, 4)]
    for fpw, wk, nw in shapes:
        for u in (1, 2, 4, 8) + ((12, 14, 16) if (fpw, wk, nw) == (1, 1, 8) else ()):
            fb = fpw * nw // wk
            out.append(dict(name="spmm_rowblock_kernel<%d, %d, %d, %d, false>" % (fpw, wk, u, nw), family="synthetic", kernel="rowblock",
                            options=dict(rowblock_fpw=fpw, rowblock_many_fpw=fpw, rowblock_wk=wk, rowblock_waves=nw, rowblock_unroll=u, rowone=0),
                            prepare=False, fb=fb, nvars=_nvars(fb), nbatch=[1, 2, 3, 33], batch_nvar=fb + 1,
                            entry="apply_many_device", unroll=u, wk=wk))
    return out


def _rowone():
    out = []
    for nw, us in ((4, (8, 12, 14)), (8, (8, 12, 14, 16))):
        for u in us:
            out.append(dict(name="spmm_rowone_kernel<%d, %d>" % (nw, u), family="synthetic", kernel="rowblock",
                            options=dict(rowone=1, rowone_waves=nw, rowone_unroll=u, rowblock_fpw=1, rowblock_wk=1),
                            prepare=False, fb=nw, nvars=_nvars(nw), nbatch=[], entry="apply_device", unroll=u, wk=1))
    return out


def _shortrow():
    out = []
    for nt in (True, False):
        for g in (4, 8, 16):
            for ra in (False, True):
                for xt in (False, True):
                    tf = lambda b: "true" if b else "false"
                    out.append(dict(name="spmm_shortrow_kernel<%s, %d, %s, %s>" % (tf(nt), g, tf(ra), tf(xt)), family="synthetic",
                                    kernel="shortrow",
                                    options=dict(shortrow_nt=int(nt), shortrow_group=g, shortrow_fper=16, shortrow_realign=int(ra),
                                                 shortrow_xt=int(xt)),
                                    prepare=False, fb=16, nvars=_nvars(16), nbatch=[1, 2, 3, 33], batch_nvar=17,
                                    entry="apply_many_device"))
    return out


def _rowdual():
    out = []
    for fpw in (1, 2, 4):
        for u in (1, 2, 4, 8):
            out.append(dict(name="spmm_rowblock_kernel<%d, 1, %d, 4, true>" % (fpw, u), family="g20", kernel="rowdual",
                            options=dict(rowdual_fpw=fpw, rowdual_unroll=u, rowdual_min_work=1, rowgroup_auto=0),
                            prepare=True, fb=4 * fpw, nvars=_nvars(4 * fpw), nbatch=[1, 2, 33], batch_nvar=4 * fpw + 1,
                            entry="apply_many_device"))
    return out


ROWGROUP_SHAPES = [(8, 8, 32), (8, 16, 32), (4, 4, 32), (4, 8, 32), (8, 8, 64), (8, 16, 64), (4, 4, 64), (4, 8, 64), (4, 16, 64)]


def _rowgroup():
    out = []
    for nw, u, tw in ROWGROUP_SHAPES:
        opts = dict(rowgroup_waves=nw, rowgroup_unroll=u, rowgroup_tw=tw, rowgroup_form=0)
        fam = "g20" if tw == 32 else "g5" if nw == 8 else "g5_xfast"
        out.append(dict(name="spmm_rowgroup_kernel<%d, %d, %d, false>" % (nw, u, tw), family=fam,
                        kernel="rowgroup", options=opts, prepare=True, fb=nw, nvars=_nvars(nw), nbatch=[1, 2, 33],
                        batch_nvar=nw + 1, entry="apply_many_device"))
        out.append(dict(name="spmm_rowgroup_kernel<%d, %d, %d, true>" % (nw, u, tw), family="g20_coarse", kernel="rowgroup",
                        options=opts, prepare=True, fb=nw, nvars=_nvars(nw), nbatch=[], entry="apply_pair_device"))
    return out


def _grouptile():
    out = []
    for ns, seg, nw in ((16, 128, 4), (16, 256, 8), (32, 128, 4), (32, 256, 8)):
        fam = "g20" if ns == 16 else "g20_fine"
        opts = dict(rowgroup_form=1, grouptile_seg=seg)
        for pair in (False, True):
            out.append(dict(name="spmm_grouptile_kernel<16, %d, %d, %d, %s>" % (ns, seg, nw, "true" if pair else "false"), family=fam,
                            kernel="rowgroup", options=opts, prepare=True, fb=16, nvars=_nvars(16),
                            nbatch=[] if pair else [1, 2, 33], batch_nvar=17, entry="apply_pair_device" if pair else "apply_many_device"))
    return out


def _sweep():
    # FULL: whole 64-field blocks (or a lane group filled by its batches); IDENT: column = item index, every column of the matrix
    # holds exactly one item (one or two entries).  The regridder's EvI has columns of more entries, so its items are listed with
    # their columns; the "banded" matrix has none.
    out = []
    for full in (True, False):
        for ident in (True, False):
            out.append(dict(name="spmm_sweep_kernel<%s, %s, 0>" % ("true" if full else "false", "true" if ident else "false"),
                            family="banded" if ident else "g5", kernel="colsweep", options={}, prepare=True, fb=64,
                            nvars=[64, 128] if full else [1, 7, 40, 65, 130], nbatch=[1, 2, 33] if full else [1, 33],
                            batch_nvar=64 if full else 7, entry="apply_many_device"))
    return out


RECIPES = _rowblock() + _rowone() + _shortrow() + _rowdual() + _rowgroup() + _grouptile() + _sweep()
BY_NAME = {r["name"]: r for r in RECIPES}
assert len(BY_NAME) == len(RECIPES), "one recipe per instantiation"
