"""The size thresholds and fallback limits of the sorted-grid builds, one hand-built grid on each side of every one.

A plain module (no tests, no fixtures).  The sorted-grid builds are the per-range build (icebin_amd/csrc/fastasm.inl), the
streamed build (streamasm.inl) and the static plan both depend on (ensure_plan).  They choose kernel instantiations by size and
hand a build that hits a limit on to the next path, so a bitwise comparison with the oracle proves nothing about a path the grid
never reaches.  tests/test_assembly_limit_cases.py measures, with numpy and without the library, that every grid below has the
property its case claims; tests/test_gpu_assembly_limits.py runs every case on the GPU, asserts the path that built each matrix
and compares it with the oracle bit for bit; tests/test_capi_symbols.py checks that KERNELS names exactly the k_plan_* / k_fa_* /
k_sa_* kernels of the code object.

THRESHOLDS  one row per condition: where it sits (host-decided rows: the rule function of icebin_amd/csrc/asm_plan.h, checked on both
            sides by tests/cpp/test_asm_plan.cpp; limits the kernels detect: file and line), what is measured, and the value on each side ("in" / "over": any value on that side);
            INSIDE holds the predicate "inside the limit" of every row.
CASES       one dict per case:
  grid      the description build_grid takes;
  knobs     a list of variants, each a dict of process-wide set_tuning knobs the builds run under ({}: the defaults);
  builds    (matrix, [(scale, correctA), ...], dims): dims "own" (sets of the matrix's own), "identity" (the identity set on the
            I / X side);
  path      the ibh_weighted_built_fast code every build must report: 0 the general pipeline, 1 the per-range build, 2 the
            streamed build -- one code for all variants, or a list with one per variant;
  discard   True: a build that the path before it started and discarded.  The test also runs EvI on a fresh caller-owned dimE
            and IvE on a pre-populated one, and compares the sets afterwards with the oracle's;
  reference "oracle" or "general" (the general pipeline, itself oracle-pinned, forced with assemble_fast=0: the 8 M-cell case);
  covers    {threshold: measured value, or "in" / "over": the side only} -- where the grid sits against each row.
"""
import numpy as np

TINY = 1e-290                          # k_plan_ifirst: a nonzero |area| below this disables the static per-ice-cell counts

# name -> (where, what is measured, value inside the limit, value beyond it; "in" / "over": any value on that side)
THRESHOLDS = {
    "sorted": ("fastasm.inl:66 k_plan_flags", "adjacent (iA, iI) pairs out of order", 0, 1),
    "nhc": ("fastasm.inl:170 ensure_plan (the streamed build: asm_plan.h plan_stream)", "elevation classes (nhc <= FA_NC = 64)", 64, 65),
    "ilmax": ("fastasm.inl:99 k_plan_ifirst", "exchange cells of one ice cell (<= FA_ILMAX = 8)", 8, 9),
    "dupmax": ("fastasm.inl:82 k_plan_ranges", "longest run of one (iA, iI) pair (<= FA_DUPMAX = 4)", 4, 5),
    "tiny": ("fastasm.inl:109 k_plan_ifirst", "smallest nonzero |area| (>= 1e-290 keeps the static counts)", TINY, np.nextafter(TINY, 0.0)),
    "rel32_ep": ("asm_plan.h stream_rel32", "2 * longest range (elevation-class builds; <= 65535: 16-bit positions)", 65534, 65536),
    "rel32": ("asm_plan.h stream_rel32", "longest range (builds without classes; <= 65535: 16-bit positions)", 65535, 65536),
    "emit_blocks": ("asm_plan.h stream_emit_grid (EMIT_BLOCKS)", "exchange cells of a 32-bit-position grid (<= 8192 workgroups x 1024 cells)", "in", "over"),
    "oldseg_s": ("streamasm.inl:357 k_sa_ranges / :261 k_sa_rangecounts", "straddlers of one (range, class) segment, small table (<= 128)", 128, 129),
    "oldseg_l": ("streamasm.inl:357 k_sa_ranges / :261 k_sa_rangecounts", "straddlers of one (range, class) segment, large table (<= 512)", 512, 513),
    "default_oldseg": ("asm_plan.h stream_oldseg", "mean range length (<= 2048: the small straddler table)", "in", "over"),
    "default_wpr4": ("asm_plan.h stream_wpr", "mean range length (<= 1024: one wave per range)", "in", "over"),
    "default_wpr16": ("asm_plan.h stream_wpr", "mean range length (<= 4096: four waves per range)", "in", "over"),
    "default_rowsl": ("asm_plan.h stream_rowsl", "ranges (< 16384: no lane-parallel row kernel)", "in", "over"),
    "fa_oldmax": ("fastasm.inl:648 k_fa_count / :1167 k_fa_range", "straddling entries of one range (<= FA_OLDMAX = 512)", 512, 513),
    "lcap_s0": ("fastasm.inl:984 k_fa_range<128, 2>", "entries of one range (<= LCAP = 1024: values in LDS)", 1024, 1025),
    "lcap_s1": ("fastasm.inl:984 k_fa_range<256, 4>", "entries of one range (<= LCAP = 2048)", 2048, 2049),
    "lcap_s2": ("fastasm.inl:984 k_fa_range<1024, 4>", "entries of one range (<= LCAP = 4096)", 4096, 4097),
    "lcap_s3": ("fastasm.inl:984 k_fa_range<1024, 1>", "entries of one range (<= LCAP = 4096)", 4096, 4097),
    "pass_s0": ("asm_plan.h FA_SHAPE_T x FA_SHAPE_CPT, shape 0 (128 x 2)", "range length against one pass of 256 cells", 256, 257),
    "pass_s1": ("asm_plan.h FA_SHAPE_T x FA_SHAPE_CPT, shape 1 (256 x 4)", "range length against one pass of 1024 cells", 1024, 1025),
    "pass_s2": ("asm_plan.h FA_SHAPE_T x FA_SHAPE_CPT, shape 2 (1024 x 4)", "range length against one pass of 4096 cells", 4096, 4097),
    "pass_s3": ("asm_plan.h FA_SHAPE_T x FA_SHAPE_CPT, shape 3 (1024 x 1)", "range length against one pass of 1024 cells", 1024, 1025),
    "stream_default": ("asm_plan.h stream_default", "exchange cells (< 2^20: no streamed build by default)", (1 << 20) - 1, 1 << 20),
    "optimistic": ("asm_plan.h range_optimistic", "exchange cells (<= 2^20: outputs by upper bounds, one read-back)", 1 << 20, (1 << 20) + 1),
    "chained": ("asm_plan.h range_chained", "ranges (x 1 class) of a one-class build (< 2^15: scans chained in k_fa_count)", 32767, 32768),
    "rscan_many": ("asm_plan.h range_scan_form", "ranges of an unchained build (<= 4096: k_fa_rscan in one workgroup)", 4096, 4097),
    "psums": ("asm_plan.h range_sums_form", "ice cells with several exchange cells (<= 2^20: k_fa_psums8)", "in", "over"),
    # what the entry counts above are made of (a cell between two classes has two entries)
    "entries_max": ("streamasm.inl k_sa_ranges (rel)", "most entries of one range (<= 65535: they fit 16-bit positions)", 65534, 65536),
    "rel16_used": ("streamasm.inl k_sa_ranges (rel)", "largest position a range of that many entries must hold in a 16-bit build (<= 32767: bit 15 never set)", "in", 65533),
    "two_class": ("assemble.hip make_cell (nep == 2)", "share of exchange cells with two entries (0: one class each)", 0.0, "over"),
    "weight_underflow": ("fastasm.inl:536 k_fa_count / streamasm.inl:102 sa_classes", "cells with area != 0, weight != 0, area * weight == 0 (0: the static counts hold)", 0, 1),
}
# the predicate "inside the limit" of each row, on the measured value
INSIDE = {
    "sorted": lambda v: v == 0, "nhc": lambda v: v <= 64, "ilmax": lambda v: v <= 8, "dupmax": lambda v: v <= 4,
    "tiny": lambda v: v >= TINY, "rel32_ep": lambda v: v <= 65535, "rel32": lambda v: v <= 65535,
    "emit_blocks": lambda v: v <= 8192 * 1024, "oldseg_s": lambda v: v <= 128, "oldseg_l": lambda v: v <= 512,
    "default_oldseg": lambda v: v <= 2048, "default_wpr4": lambda v: v <= 1024, "default_wpr16": lambda v: v <= 4096,
    "default_rowsl": lambda v: v < 16384, "fa_oldmax": lambda v: v <= 512,
    "lcap_s0": lambda v: v <= 1024, "lcap_s1": lambda v: v <= 2048, "lcap_s2": lambda v: v <= 4096, "lcap_s3": lambda v: v <= 4096,
    "pass_s0": lambda v: v <= 256, "pass_s1": lambda v: v <= 1024, "pass_s2": lambda v: v <= 4096, "pass_s3": lambda v: v <= 1024,
    "stream_default": lambda v: v < (1 << 20), "optimistic": lambda v: v <= (1 << 20), "chained": lambda v: v < 32768,
    "rscan_many": lambda v: v <= 4096, "psums": lambda v: v <= (1 << 20),
    "entries_max": lambda v: v <= 65535, "rel16_used": lambda v: v <= 32767, "two_class": lambda v: v == 0, "weight_underflow": lambda v: v == 0,
}
# rows whose measured property is the SET of range lengths (a grid can hold both sides at once)
PER_RANGE = {"lcap_s0", "lcap_s1", "lcap_s2", "lcap_s3", "pass_s0", "pass_s1", "pass_s2", "pass_s3"}


def build_grid(d):
    """The dict from_synthetic and orc.Regridder take, from a description (no geometry):
      ranges     length of every range (the exchange cells of atmosphere cell r, r = 0, 1, ...);
      straddle   [(r0, r1, n, cls)]: n ice cells first seen in range r0 with one more exchange cell in range r1, in class cls;
      multi      [(r0, k, n)]: n ice cells with one exchange cell in each of ranges r0 .. r0 + k - 1;
      dups       [(r, run, n)]: n ice cells with `run` exchange cells in a row in range r, all the same (iA, iI);
      nhc        elevation classes (without `elev` every ice cell sits exactly on one class: one entry per exchange cell in E);
      elev       where ice cells lie against the classes (a group spec is a class c: exactly on it, or (c0, c1, f): at
                 hcdefs[c0] + f * (hcdefs[c1] - hcdefs[c0]), two entries when 0 < f < 1):
                 {"plain": (c, f): every plain cell between classes c and c + 1 (c "cycle": ice cell % (nhc - 1)),
                  "straddle" / "multi" / "dups": one group spec (or None: as without `elev`) per entry of that list,
                  "cells": {ice cell: elevation}, the key "min_area" naming the ice cell of the area["min"] exchange cell};
      area       {"zero_every": k, "neg_every": k, "min": value}: areas 1e6 * (0.5 .. 1.5), every k-th zero / negative, and
                 one exchange cell (the middle of the last range) with the given smallest |area|;
      inversion  "first" / "last": the first / last two exchange cells swapped (the grid is sorted by (iA, iI) otherwise);
      masked     every k-th ice cell outside the elevation mask (NaN).
    Ice cells are numbered in the order they are made; the cells of every range are sorted by ice cell."""
    rng = np.random.default_rng(d.get("seed", 0))
    lengths = np.asarray(d["ranges"], np.int64)
    nR, nhc = len(lengths), int(d.get("nhc", 4))
    room = lengths.copy()
    iA_parts, iI_parts, cls = [], [], []
    group = []                             # (list, index in it) of every special ice cell
    nI = 0

    def put(r, ice, n=1):
        room[r] -= n
        assert room[r] >= 0, ("range too short for its special cells", r)
        iA_parts.append(np.full(n, r, np.int64))
        iI_parts.append(np.full(n, ice, np.int64))

    for gi, (r0, r1, n, c) in enumerate(d.get("straddle", ())):
        for _ in range(n):
            put(r0, nI); put(r1, nI); cls.append(c); group.append(("straddle", gi)); nI += 1
    for gi, (r0, k, n) in enumerate(d.get("multi", ())):
        for _ in range(n):
            for r in range(r0, r0 + k):
                put(r, nI)
            cls.append(nI % nhc); group.append(("multi", gi)); nI += 1
    for gi, (r, run, n) in enumerate(d.get("dups", ())):
        for _ in range(n):
            put(r, nI, run); cls.append(nI % nhc); group.append(("dups", gi)); nI += 1
    # every other cell: an ice cell of its own (bulk-generated: the large grids have millions)
    pair = int(d.get("pairs", 0))          # > 0: the plain cells come as duplicate pairs (two cells per ice cell)
    for r in range(nR):
        n = int(room[r])
        if pair:
            assert n % 2 == 0, r
            ice = nI + np.arange(n // 2)
            iA_parts.append(np.full(n, r, np.int64)); iI_parts.append(np.repeat(ice, 2))
            nI += n // 2
        else:
            iA_parts.append(np.full(n, r, np.int64)); iI_parts.append(nI + np.arange(n))
            nI += n
    cls = np.concatenate([np.asarray(cls, np.int64), np.arange(len(cls), nI) % nhc])
    iA, iI = np.concatenate(iA_parts), np.concatenate(iI_parts)
    o = np.lexsort((iI, iA))
    iA, iI = iA[o], iI[o]
    nX = len(iA)
    assert nX == lengths.sum()
    a = d.get("area", {})
    area = 1e6 * (0.5 + rng.random(nX))
    if a.get("zero_every"):
        area[3::a["zero_every"]] = 0.0
    if a.get("neg_every"):
        area[5::a["neg_every"]] *= -1.0
    x_min = int(lengths[:-1].sum() + lengths[-1] // 2)
    ice_min = int(iI[x_min])
    if "min" in a:
        area[x_min] = a["min"]
    if d.get("inversion") == "first":
        iA[[0, 1]], iI[[0, 1]] = iA[[1, 0]], iI[[1, 0]]
    elif d.get("inversion") == "last":
        iA[[-2, -1]], iI[[-2, -1]] = iA[[-1, -2]], iI[[-1, -2]]
    hcdefs = 100.0 * np.arange(nhc)
    em = hcdefs[cls].copy()
    e = d.get("elev")
    if e:
        def between(c0, c1, f):
            return hcdefs[c0] + f * (hcdefs[c1] - hcdefs[c0])
        if "plain" in e:
            c, f = e["plain"]
            ice = np.arange(len(group), nI)
            c0 = ice % (nhc - 1) if c == "cycle" else np.full(len(ice), c)
            em[ice] = between(c0, c0 + 1, f)
        for ice, (kind, gi) in enumerate(group):
            spec = (e.get(kind) or [None] * (gi + 1))[gi]
            if spec is not None:
                em[ice] = between(*spec) if isinstance(spec, tuple) else hcdefs[spec]
        for ice, v in e.get("cells", {}).items():
            em[ice_min if ice == "min_area" else ice] = v
    if d.get("masked"):
        em[::d["masked"]] = np.nan
    proj = 1e9 * (1.0 + rng.random(nR))
    g = dict(config="limits", nx=nI, ny=1, dx=1.0, x_fastest=False, nI=nI, nA=nR, im=nR, jm=1,
             ex_indices=np.stack([iA, iI], axis=1).astype(np.int32), ex_area=area, A_to_sparse=np.arange(nR, dtype=np.int64),
             A_native_area=proj * 1.01, A_proj_area=proj, hcdefs=hcdefs, hc_stride_A=1, hc_stride_HC=nR,
             interp_style=0, I_centroid_xy=np.zeros((nI, 2)))
    return g, em


def _fill(total, nR, special=()):
    """nR range lengths summing to total: the ranges listed in `special` {r: length} as given, the rest as even as possible."""
    lengths = np.zeros(nR, np.int64)
    rest = [r for r in range(nR) if r not in dict(special)]
    for r, n in dict(special).items():
        lengths[r] = n
    left = total - lengths.sum()
    lengths[rest] = left // len(rest)
    lengths[rest[: left % len(rest)]] += 1
    return lengths.tolist()


ALLB = [(True, True), (False, False)]
ONE = [(True, True)]
I_BUILDS = [("AvI", ALLB, "own"), ("IvA", ALLB, "own"), ("EvI", ALLB, "own"), ("IvE", ALLB, "own")]
ALL_BUILDS = I_BUILDS + [("AvX", ONE, "own"), ("XvA", ONE, "own"), ("EvX", ONE, "own"), ("XvE", ONE, "own"),
                         ("AvI", ONE, "identity"), ("EvI", ONE, "identity"), ("IvE", ONE, "identity"), ("XvE", ONE, "identity")]
STREAM = {"assemble_stream": 1}
NOSTREAM = {"assemble_stream": 0}
SMALL = dict(ranges=[40, 90, 300, 17, 256, 120], straddle=[(0, 1, 6, 1), (1, 3, 4, 2), (2, 4, 20, 0), (0, 5, 3, 3)],
             dups=[(2, 3, 5), (4, 2, 7)], multi=[(0, 3, 4)], area=dict(zero_every=13, neg_every=17))
NX20 = 1 << 20


def _nx20(dn, straddle):
    """16384 ranges (mean 64) holding 2^20 + dn exchange cells: ranges 0 and 1 long enough for `straddle` straddlers between them."""
    lengths = _fill(NX20 + dn, 16384, {0: 200, 1: 200})
    return dict(ranges=lengths, straddle=[(0, 1, straddle, 1)] if straddle else [], nhc=4)


CASES = [
    # ---- the static plan ----------------------------------------------------------------------------------------------------------
    dict(name="sorted", grid=SMALL, knobs=[{}, STREAM, dict(STREAM, assemble_stream_rows4=1), dict(STREAM, assemble_stream_rows4=0)],
         builds=ALL_BUILDS, path=[1, 2, 2, 2],
         covers={"sorted": 0, "nhc": 4, "ilmax": 3, "dupmax": 3, "tiny": "in", "default_oldseg": "in", "default_wpr4": "in",
                 "default_wpr16": "in", "default_rowsl": "in", "rel32": "in", "psums": "in", "fa_oldmax": "in", "oldseg_s": "in"}),
    dict(name="inversion_first", grid=dict(SMALL, inversion="first"), knobs=[{}], builds=I_BUILDS, path=0, covers={"sorted": 1}),
    dict(name="inversion_last", grid=dict(SMALL, inversion="last"), knobs=[{}], builds=I_BUILDS, path=0, covers={"sorted": 1}),
    dict(name="nhc64", grid=dict(SMALL, nhc=64), knobs=[{}, STREAM], builds=I_BUILDS, path=[1, 2], covers={"nhc": 64}),
    dict(name="nhc65", grid=dict(SMALL, nhc=65), knobs=[{}, STREAM], builds=I_BUILDS, path=0, covers={"nhc": 65}),
    dict(name="ilmax8", grid=dict(ranges=[30] * 10, multi=[(1, 8, 3)], straddle=[(0, 9, 2, 1)]), knobs=[{}, STREAM], builds=I_BUILDS,
         path=[1, 2], covers={"ilmax": 8}),
    dict(name="ilmax9", grid=dict(ranges=[30] * 10, multi=[(1, 9, 3)], straddle=[(0, 9, 2, 1)]), knobs=[{}, STREAM], builds=I_BUILDS,
         path=0, covers={"ilmax": 9}),
    dict(name="dup4", grid=dict(ranges=[50, 60, 70], dups=[(1, 4, 3), (2, 2, 4)], straddle=[(0, 2, 5, 2)]), knobs=[{}, STREAM],
         builds=I_BUILDS, path=[1, 2], covers={"dupmax": 4}),
    dict(name="dup5", grid=dict(ranges=[50, 60, 70], dups=[(1, 5, 1), (2, 2, 4)], straddle=[(0, 2, 5, 2)]), knobs=[{}, STREAM],
         builds=I_BUILDS, path=0, covers={"dupmax": 5}),
    # areas at the underflow cut: the streamed build takes only grids with static counts, the per-range build counts by visiting
    dict(name="area_at_cut", grid=dict(SMALL, area=dict(min=TINY)), knobs=[STREAM], builds=I_BUILDS, path=2, covers={"tiny": TINY}),
    dict(name="area_above_cut", grid=dict(SMALL, area=dict(min=np.nextafter(TINY, 1.0))), knobs=[STREAM], builds=I_BUILDS, path=2,
         covers={"tiny": np.nextafter(TINY, 1.0)}),
    dict(name="area_below_cut", grid=dict(SMALL, area=dict(min=np.nextafter(TINY, 0.0))), knobs=[STREAM, {}], builds=ALL_BUILDS, path=1,
         covers={"tiny": np.nextafter(TINY, 0.0)}),
    dict(name="area_subnormal", grid=dict(SMALL, area=dict(min=-5e-324, neg_every=17)), knobs=[STREAM], builds=I_BUILDS, path=1,
         covers={"tiny": 5e-324}),
    # ---- the streamed build ---------------------------------------------------------------------------------------------------------
    dict(name="rel32_ep_in", grid=dict(ranges=[300, 32767, 700, 2000], straddle=[(0, 1, 30, 1), (1, 3, 40, 2), (1, 2, 12, 0)]),
         knobs=[STREAM], builds=ALL_BUILDS, path=2, covers={"rel32_ep": 65534, "rel32": 32767, "default_wpr16": 8941}),
    dict(name="rel32_ep_out", grid=dict(ranges=[300, 32768, 700, 2000], straddle=[(0, 1, 30, 1), (1, 3, 40, 2), (1, 2, 12, 0)]),
         knobs=[STREAM, dict(STREAM, assemble_stream_wpr=1), dict(STREAM, assemble_stream_wpr=4)], builds=ALL_BUILDS, path=2,
         covers={"rel32_ep": 65536, "rel32": 32768, "emit_blocks": 35768}),
    dict(name="rel32_in", grid=dict(ranges=[300, 65535, 700, 2000], straddle=[(0, 1, 30, 1), (1, 3, 40, 2)]),
         knobs=[STREAM], builds=ALL_BUILDS, path=2, covers={"rel32": 65535}),
    dict(name="rel32_out", grid=dict(ranges=[300, 65536, 700, 2000], straddle=[(0, 1, 30, 1), (1, 3, 40, 2)], dups=[(1, 4, 9)]),
         knobs=[STREAM, dict(STREAM, assemble_stream_rowsl=1)], builds=ALL_BUILDS, path=2, covers={"rel32": 65536}),
    dict(name="oldseg_s_128", grid=dict(ranges=[400, 500, 300], straddle=[(0, 1, 128, 1), (1, 2, 20, 2)]), knobs=[STREAM],
         builds=I_BUILDS, path=2, covers={"oldseg_s": 128, "default_oldseg": 400}),
    dict(name="oldseg_s_129", grid=dict(ranges=[400, 500, 300], straddle=[(0, 1, 129, 1), (1, 2, 20, 2)]), knobs=[STREAM],
         builds=I_BUILDS, path=1, discard=True, covers={"oldseg_s": 129}),
    dict(name="oldseg_l_512", grid=dict(ranges=[2600, 2600], straddle=[(0, 1, 512, 1)]), knobs=[STREAM], builds=I_BUILDS, path=2,
         covers={"oldseg_l": 512, "default_oldseg": 2600, "default_wpr4": 2600}),
    dict(name="oldseg_l_513", grid=dict(ranges=[2600, 2600], straddle=[(0, 1, 513, 1)]), knobs=[STREAM], builds=I_BUILDS, path=0,
         discard=True, covers={"oldseg_l": 513}),
    dict(name="oldseg_l_forced_512", grid=dict(ranges=[600, 700], straddle=[(0, 1, 512, 1)]),
         knobs=[dict(STREAM, assemble_stream_oldseg=512)], builds=I_BUILDS, path=2, covers={"oldseg_l": 512, "default_oldseg": "in"}),
    dict(name="oldseg_l_forced_513", grid=dict(ranges=[600, 700], straddle=[(0, 1, 513, 1)]),
         knobs=[dict(STREAM, assemble_stream_oldseg=512)], builds=I_BUILDS, path=0, discard=True, covers={"oldseg_l": 513}),
    # ---- the per-range build --------------------------------------------------------------------------------------------------------
    dict(name="fa_oldmax_512", grid=dict(ranges=[600, 700], straddle=[(0, 1, 300, 1), (0, 1, 212, 2)]), knobs=[NOSTREAM],
         builds=I_BUILDS, path=1, covers={"fa_oldmax": 512}),
    dict(name="fa_oldmax_513", grid=dict(ranges=[600, 700], straddle=[(0, 1, 300, 1), (0, 1, 213, 2)]), knobs=[NOSTREAM],
         builds=I_BUILDS, path=0, discard=True, covers={"fa_oldmax": 513}),
    dict(name="lcap_and_passes",
         grid=dict(ranges=[255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097], nhc=6,
                   straddle=[(0, 3, 40, 1), (4, 9, 60, 2), (7, 11, 30, 3)]),
         knobs=[dict(NOSTREAM, assemble_range_shape=s) for s in range(4)] + [dict(NOSTREAM, assemble_range_shape=1, assemble_static_count=0)],
         builds=ALL_BUILDS, path=1,
         covers={"lcap_s0": 1024, "lcap_s1": 2048, "lcap_s2": 4096, "lcap_s3": 4096, "pass_s0": 256, "pass_s1": 1024, "pass_s2": 4096,
                 "pass_s3": 1024}),
    dict(name="lcap_and_passes_over", grid=dict(ranges=[255, 1025, 2049, 4097, 257], nhc=3, straddle=[(0, 3, 40, 1), (1, 2, 60, 2)]),
         knobs=[dict(NOSTREAM, assemble_range_shape=s) for s in range(4)], builds=I_BUILDS, path=1,
         covers={"lcap_s0": 1025, "lcap_s1": 2049, "lcap_s2": 4097, "lcap_s3": 4097, "pass_s0": 257, "pass_s1": 1025, "pass_s2": 4097,
                 "pass_s3": 1025}),
    # ---- dispatch by size (default knobs) --------------------------------------------------------------------------------------------
    dict(name="nx_2p20_minus_1", grid=_nx20(-1, 0), knobs=[{}], builds=I_BUILDS, path=1,
         covers={"stream_default": NX20 - 1, "default_rowsl": 16384}),
    dict(name="nx_2p20", grid=_nx20(0, 0), knobs=[{}], builds=I_BUILDS + [("XvE", ONE, "own")], path=2,
         covers={"stream_default": NX20, "optimistic": NX20, "default_rowsl": 16384}),
    dict(name="nx_2p20_discard", grid=_nx20(0, 129), knobs=[{}], builds=I_BUILDS, path=1, discard=True,
         covers={"optimistic": NX20, "oldseg_s": 129}),
    dict(name="nx_2p20_plus_1_discard", grid=_nx20(1, 129), knobs=[{}], builds=I_BUILDS, path=1, discard=True,
         covers={"optimistic": NX20 + 1, "oldseg_s": 129}),
    dict(name="chained_32767", grid=dict(ranges=[2] * 32767, nhc=2), knobs=[{}], builds=I_BUILDS, path=1, covers={"chained": 32767}),
    dict(name="chained_32768", grid=dict(ranges=[2] * 32768, nhc=2), knobs=[{}], builds=I_BUILDS, path=1, covers={"chained": 32768}),
    dict(name="rscan_4096", grid=dict(ranges=[3] * 4096, nhc=8, straddle=[(0, 4095, 1, 1)]), knobs=[{}],
         builds=I_BUILDS + [("EvX", ONE, "own"), ("XvE", ONE, "own")], path=1, covers={"rscan_many": 4096}),
    dict(name="rscan_4097", grid=dict(ranges=[3] * 4097, nhc=8, straddle=[(0, 4096, 1, 1)]), knobs=[{}],
         builds=I_BUILDS + [("EvX", ONE, "own"), ("XvE", ONE, "own")], path=1, covers={"rscan_many": 4097}),
    # 129 ranges of 65536 cells, every ice cell a duplicate pair: 32-bit positions, the emit pass at its workgroup cap, and 2^22
    # ice cells with several exchange cells (the per-range build's column sums by k_fa_pelem)
    dict(name="emit_blocks_and_psums", grid=dict(ranges=[65536] * 129, nhc=3, pairs=1), knobs=[{}, NOSTREAM],
         builds=[(n, ONE, "own") for n, _, _ in I_BUILDS],
         path=[2, 1], reference="general", covers={"emit_blocks": 129 * 65536, "psums": 129 * 32768, "rel32": 65536}),
]

# ---- the same limits in ENTRIES: ice cells between two classes have two entries in the E-keyed matrices (make_cell, nep == 2) ------
TWO = dict(plain=("cycle", 0.25))          # every plain cell a quarter of the way from its class to the next: weights 0.75 / 0.25
_SHAPES = [dict(NOSTREAM, assemble_range_shape=s) for s in range(4)] + [dict(NOSTREAM, assemble_range_shape=1, assemble_static_count=0)]
_WPRS = [STREAM, dict(STREAM, assemble_stream_wpr=1), dict(STREAM, assemble_stream_wpr=4)]
_LONG = [(0, 1, 30, 1), (1, 3, 40, 2), (1, 2, 12, 0)]
_LONG2 = dict(TWO, straddle=[(1, 2, 0.5), (2, 3, 0.25), (0, 1, 0.75)])
E_BUILDS = I_BUILDS + [("EvX", ONE, "own"), ("XvE", ONE, "own")]
EI_BUILDS = [("EvI", ALLB, "own"), ("IvE", ALLB, "own")]
E_OF_ALL = [b for b in ALL_BUILDS if "E" in b[0]]         # the matrices of ALL_BUILDS with elevation classes
# SMALL with one exchange cell of area 1e-280 (above the cut: the plan keeps its static counts), its ice cell at `e`.  The oracle's
# EvI / EvX hold 806 / 823 entries with e = 1e-60 as with e = 0, and 807 / 824 with e = 1e-40.
_under = lambda e: dict(SMALL, area=dict(min=1e-280), elev=dict(cells={"min_area": e}))
# SMALL at the ends of the class table: every plain cell between two classes (62 / 63 among them), the groups on 63, on 0, between
# 62 and 63 and between 0 and 1 -- the class bytes 62 | 2 << 6 and 63 | 1 << 6 next to the sentinels 0xFD .. 0xFF
_ENDS = dict(plain=("cycle", 0.5), straddle=[(62, 63, 0.5), 63, 0, (0, 1, 0.5)], dups=[(62, 63, 0.25), 0], multi=[63])
CASES += [
    # the long range two-class throughout: 65 534 entries in 16-bit positions (the last one 65 533), 65 536 in 32-bit ones
    dict(name="rel32_ep_in_two", grid=dict(ranges=[300, 32767, 700, 2000], straddle=_LONG, elev=_LONG2), knobs=_WPRS, builds=ALL_BUILDS,
         path=2, covers={"rel32_ep": 65534, "entries_max": 65534, "rel16_used": 65533, "two_class": 1.0, "weight_underflow": 0}),
    dict(name="rel32_ep_out_two", grid=dict(ranges=[300, 32768, 700, 2000], straddle=_LONG, elev=_LONG2), knobs=_WPRS, builds=ALL_BUILDS,
         path=2, covers={"rel32_ep": 65536, "entries_max": 65536, "rel16_used": 0, "emit_blocks": 35768}),
    # 65 535 cells: the builds without classes keep 16-bit positions, the class builds of the same grid hold 131 070 entries
    dict(name="rel32_in_two", grid=dict(ranges=[300, 65535, 700, 2000], straddle=_LONG[:2], elev=_LONG2), knobs=[STREAM], builds=ALL_BUILDS,
         path=2, covers={"rel32": 65535, "rel32_ep": "over", "entries_max": 131070}),
    # LCAP counts entries, the passes count cells: ranges of 512 / 1024 / 2048 two-class cells sit ON every LCAP, one cell more is
    # beyond it while a pass of shape 2 (4096 cells) or 3 (1024) still holds the range; 511 two-class + 2 on-class cells make 1024
    # entries, 512 + 1 make the odd 1025 (the on-class cells: `dups` runs of one cell)
    dict(name="lcap_entries", grid=dict(ranges=[512, 1024, 2048, 513, 300], nhc=5, dups=[(3, 1, 2)], straddle=[(0, 4, 20, 1), (1, 4, 30, 2)],
                                        elev=dict(TWO, dups=[2], straddle=[(1, 2, 0.5), (2, 3, 0.5)])),
         knobs=_SHAPES, builds=ALL_BUILDS, path=1,
         covers={"lcap_s0": 1024, "lcap_s1": 2048, "lcap_s2": 4096, "lcap_s3": 4096, "pass_s0": 512, "pass_s1": 513, "pass_s2": 2048,
                 "pass_s3": 513}),
    dict(name="lcap_entries_over", grid=dict(ranges=[513, 1025, 2049, 514, 300], nhc=5, dups=[(3, 1, 1)], straddle=[(0, 4, 20, 1), (1, 4, 30, 2)],
                                             elev=dict(TWO, dups=[2], straddle=[(1, 2, 0.5), (2, 3, 0.5)])),
         knobs=_SHAPES, builds=ALL_BUILDS, path=1,
         covers={"lcap_s0": 1026, "lcap_s1": 2050, "lcap_s2": 4098, "lcap_s3": 4098, "pass_s0": 513, "pass_s1": 1025, "pass_s2": 2049,
                 "pass_s3": 1025}),
    dict(name="lcap_entries_odd", grid=dict(ranges=[513, 300], nhc=5, dups=[(0, 1, 1)], elev=dict(TWO, dups=[2])), knobs=_SHAPES,
         builds=E_BUILDS, path=1, covers={"lcap_s0": 1025, "pass_s0": 513, "pass_s1": 513}),
    # 256 two-class straddlers are 512 straddling entries; one on-class straddler more is 513 (EvI and IvE only: AvI and IvA have 257 straddlers
    # there, and on exchange-cell keys nothing straddles: those stay with the per-range build)
    dict(name="fa_oldmax_512_two", grid=dict(ranges=[600, 700], straddle=[(0, 1, 256, 1)], elev=dict(straddle=[(1, 2, 0.5)])), knobs=[NOSTREAM],
         builds=I_BUILDS, path=1, covers={"fa_oldmax": 512}),
    dict(name="fa_oldmax_513_two", grid=dict(ranges=[600, 700], straddle=[(0, 1, 256, 1), (0, 1, 1, 2)], elev=dict(straddle=[(1, 2, 0.5), None])),
         knobs=[NOSTREAM], builds=EI_BUILDS, path=0, discard=True, covers={"fa_oldmax": 513}),
    # n two-class straddlers between classes 1 and 2 fill the segments of both; one on-class straddler of class 2 more and only the
    # UPPER class's segment is over
    dict(name="oldseg_s_128_two", grid=dict(ranges=[400, 500, 300], straddle=[(0, 1, 128, 1), (1, 2, 20, 2)], elev=dict(straddle=[(1, 2, 0.5), None])),
         knobs=[STREAM], builds=I_BUILDS, path=2, covers={"oldseg_s": 128, "default_oldseg": 400, "rel16_used": "in", "entries_max": "in"}),
    dict(name="oldseg_s_129_two", grid=dict(ranges=[400, 500, 300], straddle=[(0, 1, 128, 1), (1, 2, 20, 2), (0, 1, 1, 2)],
                                            elev=dict(straddle=[(1, 2, 0.5), None, None])),
         knobs=[STREAM], builds=I_BUILDS, path=1, discard=True, covers={"oldseg_s": 129}),
    dict(name="oldseg_l_512_two", grid=dict(ranges=[2600, 2600], straddle=[(0, 1, 512, 1)], elev=dict(straddle=[(1, 2, 0.5)])), knobs=[STREAM],
         builds=I_BUILDS, path=2, covers={"oldseg_l": 512, "default_oldseg": 2600, "default_wpr4": 2600}),
    dict(name="oldseg_l_513_two", grid=dict(ranges=[2600, 2600], straddle=[(0, 1, 512, 1), (0, 1, 1, 2)], elev=dict(straddle=[(1, 2, 0.5), None])),
         knobs=[STREAM], builds=I_BUILDS, path=0, discard=True, covers={"oldseg_l": 513}),
    dict(name="oldseg_l_forced_512_two", grid=dict(ranges=[600, 700], straddle=[(0, 1, 512, 1)], elev=dict(straddle=[(1, 2, 0.5)])),
         knobs=[dict(STREAM, assemble_stream_oldseg=512)], builds=I_BUILDS, path=2, covers={"oldseg_l": 512, "default_oldseg": "in"}),
    dict(name="oldseg_l_forced_513_two", grid=dict(ranges=[600, 700], straddle=[(0, 1, 512, 1), (0, 1, 1, 2)], elev=dict(straddle=[(1, 2, 0.5), None])),
         knobs=[dict(STREAM, assemble_stream_oldseg=512)], builds=I_BUILDS, path=0, discard=True, covers={"oldseg_l": 513}),
    # the ice cells in several ranges and the duplicate runs two-class: a merged run sums both entries
    dict(name="ilmax8_two", grid=dict(ranges=[30] * 10, multi=[(1, 8, 3)], straddle=[(0, 9, 2, 1)], elev=dict(multi=[(1, 2, 0.25)], straddle=[(0, 1, 0.5)])),
         knobs=[{}, STREAM], builds=E_BUILDS, path=[1, 2], covers={"ilmax": 8, "two_class": "over"}),
    dict(name="ilmax9_two", grid=dict(ranges=[30] * 10, multi=[(1, 9, 3)], straddle=[(0, 9, 2, 1)], elev=dict(multi=[(1, 2, 0.25)], straddle=[(0, 1, 0.5)])),
         knobs=[{}, STREAM], builds=E_BUILDS, path=0, covers={"ilmax": 9, "two_class": "over"}),
    dict(name="dup4_two", grid=dict(ranges=[50, 60, 70], dups=[(1, 4, 3), (2, 2, 4)], straddle=[(0, 2, 5, 2)], elev=dict(dups=[(0, 1, 0.25), (2, 3, 0.5)])),
         knobs=[{}, STREAM], builds=E_BUILDS, path=[1, 2], covers={"dupmax": 4, "two_class": "over"}),
    dict(name="dup5_two", grid=dict(ranges=[50, 60, 70], dups=[(1, 5, 1), (2, 2, 4)], straddle=[(0, 2, 5, 2)], elev=dict(dups=[(0, 1, 0.25), (2, 3, 0.5)])),
         knobs=[{}, STREAM], builds=E_BUILDS, path=0, covers={"dupmax": 5, "two_class": "over"}),
    dict(name="nhc64_ends", grid=dict(SMALL, nhc=64, elev=_ENDS), knobs=[{}, STREAM], builds=ALL_BUILDS, path=[1, 2],
         covers={"nhc": 64, "two_class": "over"}),
    dict(name="nhc65_ends", grid=dict(SMALL, nhc=65, elev=_ENDS), knobs=[{}, STREAM], builds=I_BUILDS, path=0, covers={"nhc": 65}),
    # area * weight underflows: the oracle drops the entry, the class pattern of the elevation still says two.  The static counts of
    # both fast builds are (classes of the elevation) x (cells with an area), so neither may build this grid: the streamed build
    # refuses a mask with a weight below 1e-30 (times the plan's smallest area, 1e-290, that is the smallest product it could
    # not tell from zero), the per-range build raises a fallback flag where it meets the underflow -- path 0, whatever the knobs.
    # (The matrices with classes: the others multiply no weights and keep their fast builds.)
    dict(name="weight_underflow", grid=_under(1e-60), knobs=[{}, STREAM, NOSTREAM], builds=E_OF_ALL, path=0, discard=True,
         covers={"weight_underflow": 1, "tiny": 1e-280}),
    dict(name="weight_underflow_plain", grid=_under(1e-60), knobs=[{}, STREAM, NOSTREAM], builds=[b for b in ALL_BUILDS if "E" not in b[0]],
         path=[1, 2, 1], covers={"weight_underflow": 1}),
    # ... the product a subnormal (1e-280 * 1e-42): the entry stays.  The streamed build hands the mask on (weight below 1e-30),
    # the per-range build meets no underflow and builds it.
    dict(name="weight_subnormal", grid=_under(1e-40), knobs=[{}, STREAM, NOSTREAM], builds=E_OF_ALL, path=1, discard=True,
         covers={"weight_underflow": 0, "tiny": 1e-280}),
    dict(name="weight_on_class", grid=_under(0.0), knobs=[{}, STREAM, NOSTREAM], builds=ALL_BUILDS, path=[1, 2, 1],
         covers={"weight_underflow": 0, "two_class": 0.0, "tiny": 1e-280}),
]

# the shared (several-rank) streamed build of a 32-bit-position grid: tests/test_distributed_gloo.py's worker, config "limits:<case>"
SHARDED_CASE = "rel32_out"

# every k_plan_* / k_fa_* / k_sa_* kernel of assemble.o, as the demangler spells it inside namespace ibh -> a test that launches it
_T = "test_gpu_assembly_limits.py::"
_GLOO = "test_distributed_gloo.py::test_sharded_assembly_is_the_single_rank_build_bitwise"
KERNELS = {}
for _k in ("k_plan_flags", "k_plan_ranges", "k_plan_ikeys", "k_plan_ifirst", "k_plan_bits2", "k_plan_pairflags", "k_plan_pairs", "k_plan_mlist"):
    KERNELS[_k] = _T + "test_sorted_grid_limits[sorted]"
for _ep in ("false", "true"):
    for _shape in ("128, 2", "256, 4", "1024, 4", "1024, 1"):
        KERNELS["k_fa_count<%s, %s>" % (_ep, _shape)] = _T + "test_sorted_grid_limits[lcap_and_passes]"
        for _em in ("false", "true"):
            KERNELS["k_fa_range<%s, %s, %s>" % (_ep, _em, _shape)] = _T + "test_sorted_grid_limits[lcap_and_passes]"
    KERNELS["k_fa_pelem<%s, 0, false>" % _ep] = _T + "test_sorted_grid_limits[emit_blocks_and_psums]"
    KERNELS["k_fa_pelem<%s, 1, false>" % _ep] = _T + "test_sorted_grid_limits[chained_32768]"
    KERNELS["k_fa_pelem<%s, 2, false>" % _ep] = _T + "test_sorted_grid_limits[sorted]"
    KERNELS["k_fa_psums8<%s>" % _ep] = _T + "test_sorted_grid_limits[nx_2p20_plus_1_discard]"
    KERNELS["k_sa_flags<%s>" % _ep] = _T + "test_sorted_grid_limits[sorted]"
    for _gr in ("false", "true"):
        KERNELS["k_sa_emit<%s, %s, unsigned short, 1>" % (_ep, _gr)] = _T + "test_sorted_grid_limits[sorted]"
        KERNELS["k_sa_emit<%s, %s, unsigned int, 4>" % (_ep, _gr)] = _T + "test_sorted_grid_limits[rel32_out]"
        KERNELS["k_sa_pairs<%s, %s>" % (_ep, _gr)] = _T + "test_sorted_grid_limits[sorted]"
KERNELS["k_fa_pelem<true, 2, true>"] = _T + "test_sorted_grid_limits[oldseg_s_129]"
for _rt in ("unsigned short", "unsigned int"):
    for _w in (1, 4, 16):
        KERNELS["k_sa_ranges<true, %s, %d>" % (_rt, _w)] = _T + ("test_sorted_grid_limits[rel32_ep_out]" if _rt == "unsigned int" else
                                                                 "test_sorted_grid_limits[%s]" % {1: "sorted", 4: "oldseg_l_512", 16: "rel32_ep_in"}[_w])
KERNELS.update({
    "k_fa_count_stream<4>": _T + "test_sorted_grid_limits[nx_2p20_discard]",
    "k_fa_count_fin": _T + "test_sorted_grid_limits[nx_2p20_discard]",
    "k_fa_zero_counts": _T + "test_sorted_grid_limits[nx_2p20_discard]",
    "k_fa_init": _T + "test_sorted_grid_limits[sorted]",
    "k_fa_init_ring": _T + "test_sorted_grid_limits[sorted]",
    "k_fa_rscan": _T + "test_sorted_grid_limits[rscan_4096]",
    "k_fa_rscan_tiles": _T + "test_sorted_grid_limits[rscan_4097]",
    "k_fa_rscan_sums": _T + "test_sorted_grid_limits[rscan_4097]",
    "k_fa_rscan_apply": _T + "test_sorted_grid_limits[rscan_4097]",
    "k_fa_zero_identity": _T + "test_sorted_grid_limits[nx_2p20_discard]",
    "k_sa_rangecounts": _T + "test_sorted_grid_limits[sorted]",
    "k_sa_oldsort<128>": _T + "test_sorted_grid_limits[nx_2p20]",
    "k_sa_oldsort<512>": _T + "test_sorted_grid_limits[rel32_out]",
    "k_sa_rows1<false, 128>": _T + "test_sorted_grid_limits[sorted]",
    "k_sa_rows1<true, 128>": _T + "test_sorted_grid_limits[dup4]",
    "k_sa_rows1<false, 512>": _T + "test_sorted_grid_limits[oldseg_l_512]",
    "k_sa_rows1<true, 512>": _T + "test_sorted_grid_limits[oldseg_l_512]",
    "k_sa_rows<false, 128, 4>": _T + "test_sorted_grid_limits[sorted]",
    "k_sa_rows<true, 128, 4>": _T + "test_sorted_grid_limits[sorted]",
    "k_sa_rowsL<false>": _T + "test_sorted_grid_limits[nx_2p20]",
    "k_sa_rowsL<true>": _T + "test_sorted_grid_limits[rel32_out]",
    "k_sa_set_u32": _T + "test_sharded_streamed_build_of_32_bit_positions",
    "k_sa_shift": _T + "test_sharded_streamed_build_of_32_bit_positions",
    "k_sa_slice_counts": _T + "test_sharded_streamed_build_of_32_bit_positions",
    "k_sa_pack_keys": _GLOO,
    "k_sa_pack_rows": _GLOO,
    "k_sa_pack_mw": _GLOO,
    "k_sa_pack_mw_g": _GLOO,
    "k_sa_unpack_rows": _GLOO,
    "k_sa_unpack_mw": _GLOO,
    "k_sa_unpack_rli": _GLOO,
})

# instantiated but unreachable: kernel -> why no build launches it (test_capi_symbols.py accepts these and no others)
UNREACHABLE = {
    # a pre-populated column set is an E set (fast_build), and every matrix with E keys is an elevation-class build (EP = true):
    # the EP = false instantiation of the per-row selection branch (fastasm.inl fa_launch_pemit) is dead
    "k_fa_pelem<false, 2, true>": "pre-populated G sets are E sets, and E-key builds are always elevation-class (EP) builds",
}
