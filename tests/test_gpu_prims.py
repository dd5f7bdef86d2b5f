"""The assembly's integer primitives (prims.hip) against exact numpy references, at their tile, window, grid-cap and wrap edges.

Every kernel of prims.o runs here through the ibh_selftest_* entries (tests/prims_kernel_cases.py names the case of each):
  - the one-launch look-back scan over u32 and u8 (SC_TILE = 2048, 64-tile look-back windows, 32-bit wrap of the sums), and the
    life of its per-thread status buffer (allocation, growth, the 30-bit epoch rollover);
  - the three-channel scan (21-bit channels packed in a u64, a single-workgroup middle pass that loops past 1024 tiles);
  - the device-wide radix sort (RS_TILE = 4096, fields split into passes of <= 8 bits, ballot ranking, stability with arbitrary
    bits outside the sorted fields);
  - the adaptive ordering (pieces of 2 .. 8192 in three LDS size classes, grid caps of 3072 / 1024 / 512 workgroups, the
    flags-only analysis followed by the radix sort).
Every result is compared with np.array_equal; the selftests also fail when a primitive writes past its output."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

from icebin_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prims_kernel_cases  # noqa: E402,F401  (the kernel -> case table checked by test_capi_symbols.py)

pytestmark = pytest.mark.gpu

SC_TILE, RS_TILE = 2048, 4096
IN_PLACE, FRESH_STATE, NEAR_WRAP = 1, 2, 4
U32, U8, SCAN3 = 0, 1, 2
M32 = np.uint64(0xFFFFFFFF)


# ---- entry points ----------------------------------------------------------------------------------------------------------
def run_scan(kind, x, flags=0):
    n = len(x)
    out = np.full(3 * n if kind == SCAN3 else n, 0x5A5A5A5A, np.uint32)
    tot = np.full(3, 0x5A5A5A5A, np.uint32)
    _capi.check(_capi.lib().ibh_selftest_scan(kind, x.ctypes.data, n, out.ctypes.data, tot.ctypes.data, flags))
    return out, (tot if kind == SCAN3 else tot[0])


def run_radix(keys, fields):
    n = len(keys)
    f = np.ascontiguousarray(np.asarray(fields, np.int32).reshape(-1))
    kout, perm = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    _capi.check(_capi.lib().ibh_selftest_radix_sort(keys.ctypes.data, n, f.ctypes.data, len(fields), kout.ctypes.data, perm.ctypes.data))
    return kout, perm


def run_order(keys, lo_bits, hi_bits, try_pieces):
    n = len(keys)
    perm, info, path = np.zeros(n, np.uint32), np.zeros(6, np.uint32), C.c_int(-1)
    _capi.check(_capi.lib().ibh_selftest_order(keys.ctypes.data, n, lo_bits, hi_bits, try_pieces, perm.ctypes.data, info.ctypes.data,
                                               C.byref(path)))
    return perm, dict(zip(("flags", "nchunks", "maxlen", "nsmall", "nmid", "nbig"), info.tolist())), path.value


# ---- references -------------------------------------------------------------------------------------------------------------
def ref_scan(x):
    c = np.cumsum(x, dtype=np.uint64)
    total = int(c[-1] & M32) if len(x) else 0
    return np.concatenate([np.zeros(1, np.uint64), c[:-1]]).astype(np.uint64)[:len(x)] & M32, total


def check_scan(kind, x, flags=0):
    out, tot = run_scan(kind, x, flags)
    ref, rtot = ref_scan(x)
    assert np.array_equal(out, ref), (kind, len(x), flags, int(np.argmax(out != ref)))
    assert int(tot) == rtot, (kind, len(x), flags, int(tot), rtot)


def scan3_channels(pk):
    pk = pk.astype(np.uint32)
    return [((pk & 1) + ((pk >> 1) & 1)), (((pk >> 2) & 1) + ((pk >> 3) & 1)), ((pk >> 4) & 3)]


def check_scan3(pk):
    out, tot = run_scan(SCAN3, pk)
    n = len(pk)
    for ch, x in enumerate(scan3_channels(pk)):
        ref, rtot = ref_scan(x)
        got = out[ch * n:(ch + 1) * n]
        assert np.array_equal(got, ref), (ch, n, int(np.argmax(got != ref)))
        assert int(tot[ch]) == rtot, (ch, n, int(tot[ch]), rtot)


def field_of(keys, shift, nbits):
    return (keys >> np.uint64(shift)) & np.uint64((1 << nbits) - 1)


def ref_radix(keys, fields):
    """stable LSD: one stable sort per field, least significant field first"""
    perm = np.arange(len(keys))
    for shift, nbits in fields:
        perm = perm[np.argsort(field_of(keys[perm], shift, nbits), kind="stable")]
    return perm.astype(np.uint32)


def check_radix(keys, fields):
    kout, perm = run_radix(keys, fields)
    ref = ref_radix(keys, fields)
    assert np.array_equal(np.sort(perm), np.arange(len(keys), dtype=np.uint32)), "elements lost or duplicated"
    assert np.array_equal(perm, ref), (len(keys), fields, int(np.argmax(perm != ref)))
    assert np.array_equal(kout, keys[ref]), (len(keys), fields)


def ref_pieces(keys):
    """The analysis of prims.hip: a cut at k where max(keys[0,k)) <= min(keys[k,n)); pieces of >= 2 elements between cuts."""
    n = len(keys)
    if n < 2:
        return []
    pmax = np.maximum.accumulate(keys)
    smin = np.minimum.accumulate(keys[::-1])[::-1]
    cut = np.ones(n, bool)
    cut[1:] = pmax[:-1] <= smin[1:]
    starts = np.flatnonzero(cut)
    lens = np.diff(np.append(starts, n))
    return lens[lens >= 2]


def check_order(keys, lo_bits, hi_bits, try_pieces=1, want_path=None):
    keys = np.ascontiguousarray(keys, np.uint64)
    perm, info, path = run_order(keys, lo_bits, hi_bits, try_pieces)
    ref = np.argsort(keys, kind="stable").astype(np.uint32)
    assert np.array_equal(perm, ref), (len(keys), lo_bits, hi_bits, try_pieces, int(np.argmax(perm != ref)))
    flags = 0
    if len(keys) >= 2:
        a, b = keys[:-1], keys[1:]
        flags = (1 if np.any(b < a) else 0) | (2 if np.any((b >> np.uint64(32)) < (a >> np.uint64(32))) else 0) \
            | (4 if np.any((b & M32) < (a & M32)) else 0)
    assert info["flags"] == flags, (info, flags)
    if try_pieces and len(keys) >= 2:
        lens = ref_pieces(keys)
        want = dict(flags=flags, nchunks=len(lens), maxlen=int(lens.max()) if len(lens) else 0,
                    nsmall=int(np.sum(lens <= 2048)), nmid=int(np.sum((lens > 2048) & (lens <= 4096))), nbig=int(np.sum(lens > 4096)))
        assert info == want, (info, want)
        assert path == (0 if not flags & 1 else 1 if want["maxlen"] <= 8192 else 2), (path, info)
    elif len(keys) >= 2:
        assert info == dict(flags=flags, nchunks=0, maxlen=0xFFFFFFFF, nsmall=0, nmid=0, nbig=0), info
        assert path == (0 if not flags & 1 else 2), (path, info)
    if want_path is not None:
        assert path == want_path, (path, info)
    return info


# ---- scans ------------------------------------------------------------------------------------------------------------------
SCAN_SIZES = [0, 1, 2047, 2048, 2049, 64 * 2048, 64 * 2048 + 1, 65 * 2048 + 1, 129 * 2048 + 7, (1 << 24) + 2049, (1 << 25) + 3]
BIG = (1 << 24)


def scan_values(kind, n, how, rng):
    dt, vmax = (np.uint32, 0xFFFFFFFF) if kind == U32 else (np.uint8, 255)
    if how == "zeros":
        return np.zeros(n, dt)
    if how == "ones":
        return np.ones(n, dt)
    if how == "max":
        return np.full(n, vmax, dt)
    if how == "random":
        return rng.integers(0, vmax, n, dtype=dt, endpoint=True)
    x = np.zeros(n, dt)                      # spikes: the first and last element of every tile, and the last element
    x[0::SC_TILE] = rng.integers(vmax // 2, vmax, len(x[0::SC_TILE]), dtype=dt, endpoint=True)
    x[SC_TILE - 1::SC_TILE] = rng.integers(vmax // 2, vmax, len(x[SC_TILE - 1::SC_TILE]), dtype=dt, endpoint=True)
    if n:
        x[-1] = vmax
    return x


@pytest.mark.parametrize("kind", [U32, U8], ids=["u32", "u8"])
@pytest.mark.parametrize("n", SCAN_SIZES)
def test_scan_exact(kind, n):
    rng = np.random.default_rng(n * 7 + kind)
    kinds = ["zeros", "ones", "max", "random", "spikes"] if n < BIG else ["max", "random", "spikes"]
    for how in kinds:
        check_scan(kind, scan_values(kind, n, how, rng))
    if kind == U8 and n == (1 << 25) + 3:       # 255 * n overflows 32 bits: the total and the late outputs wrap
        assert 255 * n >= 1 << 32


@pytest.mark.parametrize("n", [0, 1, 2049, 64 * 2048 + 1, 129 * 2048 + 7, (1 << 24) + 2049])
def test_scan_u32_in_place(n):
    # the radix sort scans its digit table in place (in == out on the device)
    rng = np.random.default_rng(n + 11)
    for how in ("max", "random", "spikes"):
        check_scan(U32, scan_values(U32, n, how, rng), IN_PLACE)


def test_scan_status_buffer_growth():
    # fresh buffer (8192 tiles), small, then 8194 tiles (> the buffer: reallocated and cleared), then small again: the small scans
    # must not read status words of the larger ones
    rng = np.random.default_rng(5)
    check_scan(U32, rng.integers(0, 1 << 32, 3 * SC_TILE + 1, dtype=np.uint32), FRESH_STATE)
    check_scan(U8, rng.integers(0, 256, 100 * SC_TILE + 3, dtype=np.uint8))
    check_scan(U32, rng.integers(0, 1 << 32, 8194 * SC_TILE - 5, dtype=np.uint32))
    check_scan(U32, rng.integers(0, 1 << 32, 70 * SC_TILE + 9, dtype=np.uint32))
    check_scan(U8, rng.integers(0, 256, 2 * SC_TILE, dtype=np.uint8))


def test_scan_epoch_rollover():
    # epochs 1..3 leave status words behind; the epoch is then moved to 2^30 - 2: the next scan runs at 2^30 - 1 and the three after
    # it take the rollover and run at epochs 1..3 again, over a cleared buffer (stale words of the first 1..3 would be read as valid)
    rng = np.random.default_rng(6)
    check_scan(U32, rng.integers(0, 1 << 32, 300 * SC_TILE + 1, dtype=np.uint32), FRESH_STATE)
    check_scan(U32, rng.integers(0, 1 << 32, 300 * SC_TILE + 1, dtype=np.uint32))
    check_scan(U8, rng.integers(0, 256, 300 * SC_TILE + 1, dtype=np.uint8))
    check_scan(U32, rng.integers(0, 1 << 32, 500 * SC_TILE + 3, dtype=np.uint32), NEAR_WRAP)
    check_scan(U32, rng.integers(0, 1 << 32, 300 * SC_TILE + 1, dtype=np.uint32))
    check_scan(U8, rng.integers(0, 256, 300 * SC_TILE + 1, dtype=np.uint8))
    check_scan(U32, rng.integers(0, 1 << 32, 129 * SC_TILE + 7, dtype=np.uint32))
    check_scan(U32, rng.integers(0, 1 << 32, 5, dtype=np.uint32))


# ---- three-channel scan -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2047, 2048, 2049, 64 * 2048 + 1, 129 * 2048 + 7, 1023 * 2048, 1024 * 2048, 1024 * 2048 + 1,
                               3000 * 2048 + 5])
def test_scan3_exact(n):
    rng = np.random.default_rng(n + 3)
    check_scan3(np.full(n, 0x3F, np.uint32))                                           # the largest per-tile channel sums
    check_scan3(rng.integers(0, 64, n, dtype=np.uint32))                               # the six bits that are read
    check_scan3(rng.integers(0, 1 << 32, n, dtype=np.uint32))                          # garbage in bits 6..31: ignored


# ---- radix sort -------------------------------------------------------------------------------------------------------------
FIELD_LISTS = [
    [(0, 1)], [(0, 7)], [(0, 8)], [(0, 9)], [(0, 16)], [(3, 17)], [(0, 32)], [(32, 32)], [(40, 24)],
    [(0, 20), (32, 12)], [(0, 31), (32, 31)],
    [(0, 9), (20, 5), (40, 20)],
]
FIELD_IDS = ["+".join("%d:%d" % f for f in fl) for fl in FIELD_LISTS]


def field_mask(fields):
    m = 0
    for s, b in fields:
        m |= ((1 << b) - 1) << s
    return np.uint64(m)


def radix_keys(n, fields, how, rng):
    keys = rng.integers(0, 1 << 64, n, dtype=np.uint64, endpoint=False)           # garbage in every bit outside the fields
    fm = field_mask(fields)
    if how == "equal":
        return (keys & ~fm) | (np.uint64(0x9E3779B97F4A7C15) & fm)
    if how == "two_digits":                                                         # one or two digit values per pass
        pick = rng.integers(0, 2, n).astype(bool)
        v = np.where(pick, np.uint64(0x5A5A5A5A5A5A5A5A), np.uint64(0x5B5A5A5B5A5A5A5A))
        return (keys & ~fm) | (v & fm)
    if how in ("sorted", "reversed"):
        keys = keys[ref_radix(keys, fields)]
        return keys if how == "sorted" else keys[::-1].copy()
    return keys


@pytest.mark.parametrize("fields", FIELD_LISTS, ids=FIELD_IDS)
def test_radix_sort_exact(fields):
    rng = np.random.default_rng(len(FIELD_IDS[FIELD_LISTS.index(fields)]) * 1009 + sum(b for _, b in fields))
    for n in (0, 1, 2, 3, 4095, 4096, 4097, 64 * 4096 + 1):
        for how in ("random", "equal", "sorted", "reversed", "two_digits"):
            check_radix(radix_keys(n, fields, how, rng), fields)
    check_radix(radix_keys((1 << 20) + 3, fields, "random", rng), fields)


@pytest.mark.parametrize("fields", [[(0, 9)], [(0, 20), (32, 12)], [(0, 31), (32, 31)]], ids=["0:9", "0:20+32:12", "0:31+32:31"])
def test_radix_sort_large(fields):
    rng = np.random.default_rng(77)
    for how in ("random", "two_digits"):
        check_radix(radix_keys(3_000_000, fields, how, rng), fields)


# ---- adaptive ordering ------------------------------------------------------------------------------------------------------
ORDER_BITS = [(1, 1), (8, 0), (9, 17), (20, 12), (31, 31), (32, 0)]
PIECE_LENS = [2, 2048, 2049, 4096, 4097, 8192, 8193]


def rank_to_key(r, lo_bits):
    r = np.asarray(r, np.uint64)
    return ((r >> np.uint64(lo_bits)) << np.uint64(32)) | (r & np.uint64((1 << lo_bits) - 1))


def pieces_keys(lens, lo_bits, hi_bits, rng, gap=3):
    """Keys (in rank order: rank r -> (r >> lo_bits) << 32 | low bits) of consecutive pieces of exactly the given lengths: piece j
    holds ranks in [a_j, b_j], starts with b_j and ends with a_j (no cut inside), the ranges follow each other (a cut before each
    piece), with `gap` ordered single elements between pieces.  Middles are random with duplicates."""
    space = 1 << (lo_bits + hi_bits)
    width = max(1, (space - 1) // (len(lens) * (gap + 2)))
    out, r = [], 0
    for L in lens:
        w = int(min(width, rng.integers(1, max(2, min(width, L)) + 1))) if rng.random() < 0.5 else width
        w = max(1, w)
        a, b = r, r + w
        assert b < space
        mid = rng.integers(a, b + 1, L - 2, dtype=np.uint64)
        out.append(np.concatenate([np.array([b], np.uint64), mid, np.array([a], np.uint64)]))
        r = b
        if gap and r + gap < space:
            out.append(np.array(range(r + 1, r + 1 + gap), np.uint64))      # (np.arange would round ranks above 2^53)
            r += gap
    return rank_to_key(np.concatenate(out), lo_bits)


@pytest.mark.parametrize("bits", ORDER_BITS, ids=["%d_%d" % b for b in ORDER_BITS])
def test_order_piece_size_classes(bits):
    lo_bits, hi_bits = bits
    rng = np.random.default_rng(lo_bits * 100 + hi_bits)
    for L in PIECE_LENS:            # one piece of each edge length on its own (the narrow fields hold only a few pieces)
        info = check_order(pieces_keys([L], lo_bits, hi_bits, rng, gap=0 if lo_bits + hi_bits < 4 else 1), lo_bits, hi_bits,
                           want_path=1 if L <= 8192 else 2)
        assert info["maxlen"] == L
        assert (info["nsmall"], info["nmid"], info["nbig"]) == (int(L <= 2048), int(2048 < L <= 4096), int(L > 4096))
    if lo_bits + hi_bits >= 16:     # all edge lengths in one sequence: every size class sorts pieces in the same call
        lens = [2, 2048, 2049, 4096, 4097, 8192, 2, 3]
        info = check_order(pieces_keys(lens, lo_bits, hi_bits, rng), lo_bits, hi_bits, want_path=1)
        assert (info["nsmall"], info["nmid"], info["nbig"], info["maxlen"]) == (4, 2, 2, 8192)
        check_order(pieces_keys(lens + [8193], lo_bits, hi_bits, rng), lo_bits, hi_bits, want_path=2)


@pytest.mark.parametrize("case", ["small_over_cap", "mid_over_cap", "big_over_cap"])
def test_order_more_pieces_than_the_grid_caps(case):
    # grids: small pieces <= 3072 workgroups, mid <= 1024, big <= 512; past a cap each workgroup walks the list
    rng = np.random.default_rng(hash(case) & 0xFFFF)
    if case == "small_over_cap":
        lens = rng.integers(2, 9, 100_000).tolist()
    elif case == "mid_over_cap":
        lens = [3000] * 1500
    else:
        lens = [5000] * 600
    info = check_order(pieces_keys(lens, 20, 12, rng, gap=1), 20, 12, want_path=1)
    cls = {"small_over_cap": "nsmall", "mid_over_cap": "nmid", "big_over_cap": "nbig"}[case]
    assert info[cls] == len(lens) and info[cls] > {"nsmall": 3072, "nmid": 1024, "nbig": 512}[cls]


@pytest.mark.parametrize("bits", [(20, 12), (31, 31), (9, 17)], ids=["20_12", "31_31", "9_17"])
def test_order_flags_only_then_radix(bits):
    # try_pieces = 0 (the assembly with expect_local = false): flags only, then the radix sort skips the low field when it never
    # decreases along the sequence
    lo_bits, hi_bits = bits
    rng = np.random.default_rng(lo_bits + 7 * hi_bits)
    n = 300_001
    hi = rng.integers(0, 1 << hi_bits, n, dtype=np.uint64) << np.uint64(32)
    lo = rng.integers(0, 1 << lo_bits, n, dtype=np.uint64)
    info = check_order(hi | np.sort(lo), lo_bits, hi_bits, try_pieces=0, want_path=2)
    assert not info["flags"] & 4
    info = check_order(hi | np.sort(lo)[::-1], lo_bits, hi_bits, try_pieces=0, want_path=2)
    assert info["flags"] & 4
    check_order(hi | lo, lo_bits, hi_bits, try_pieces=0, want_path=2)
    check_order(np.sort(hi | lo), lo_bits, hi_bits, try_pieces=0, want_path=0)
    check_order(pieces_keys([3, 5000, 2], lo_bits, hi_bits, rng), lo_bits, hi_bits, try_pieces=0, want_path=2)
    for n in (0, 1, 2):
        check_order(np.arange(n, dtype=np.uint64)[::-1].copy(), lo_bits, hi_bits, try_pieces=0)


def test_order_small_inputs_and_tile_straddles():
    rng = np.random.default_rng(9)
    for n in (0, 1, 2, 3):
        check_order(np.arange(n, dtype=np.uint64)[::-1].copy(), 20, 12)
    keys = np.arange(5 * 2048 + 3, dtype=np.uint64)           # pieces straddling the 2048-element analysis tiles
    for e in (2046, 2047, 4095, 6143, 8190):
        keys[e:e + 3] = keys[e:e + 3][::-1].copy()
    check_order(keys, 20, 12, want_path=1)
    check_order(rng.integers(0, 1 << 20, 2, dtype=np.uint64), 20, 0)


# ---- concurrent host threads ------------------------------------------------------------------------------------------------
def test_four_threads_run_the_primitives_concurrently():
    # each thread has its own arena and scan status buffer; calls on hipStreamPerThread overlap
    errors = []

    def work(t):
        try:
            rng = np.random.default_rng(100 + t)
            for it in range(3):
                check_scan(U32, rng.integers(0, 1 << 32, (65 + 40 * t + it) * SC_TILE + t, dtype=np.uint32), FRESH_STATE if it == 0 else 0)
                check_scan(U8, rng.integers(0, 256, 129 * SC_TILE + 7 + t, dtype=np.uint8), NEAR_WRAP if it == 1 else 0)
                check_scan3(rng.integers(0, 1 << 32, (1025 + t) * SC_TILE + 1, dtype=np.uint32))
                fields = FIELD_LISTS[(4 * t + it) % len(FIELD_LISTS)]
                check_radix(radix_keys(64 * 4096 + 1 + t, fields, "random", rng), fields)
                check_order(pieces_keys(rng.integers(2, 9000, 200).tolist(), 20, 12, rng), 20, 12)
                n = 200_001
                hi = rng.integers(0, 1 << 12, n, dtype=np.uint64) << np.uint64(32)
                check_order(hi | np.sort(rng.integers(0, 1 << 20, n, dtype=np.uint64)), 20, 12, try_pieces=0)
        except BaseException as e:      # noqa: BLE001
            errors.append((t, repr(e)[:2000]))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors

