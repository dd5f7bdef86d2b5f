"""The first-seen numbering of a key stream (sparseset.hip: spsparse::SparseSet::add_dense in stream order, and the to-dense
transforms) through ibh_selftest_number_keys, against a dict-based loop, exactly (np.array_equal):
  - stream lengths at the edges of the 256-thread blocks; one address under a contended atomicMin; a permutation;
  - the old part of the set: none, empty, an identity prefix, a table; both key widths; a stride; the `act` mask;
  - TO_DENSE and TO_DENSE_IGNORE_MISSING with a missing key; keys outside the extent with the range check on."""
import ctypes as C

import numpy as np
import pytest

from icebin_amd import _capi

pytestmark = pytest.mark.gpu

ADD_DENSE, TO_DENSE, TO_DENSE_IGNORE_MISSING = 0, 1, 2
OUT_OF_RANGE, MISSING = 1, 2
NO_SET = None


def run(keys, extent, old=NO_SET, transform=ADD_DENSE, act=None, stride=1, check_range=0, dtype=np.int64):
    """old: NO_SET, ("identity", n_old) or a list of sparse keys.  Returns dense[n], the set's table afterwards (None without a
    set), n_new and the status bits."""
    keys = np.asarray(keys, dtype)
    n = len(keys)
    stream = np.full(max((n - 1) * stride + 1, 1), -7, dtype)        # (the gaps of a strided stream are never read as keys)
    stream[:n * stride:stride][:n] = keys
    if old is NO_SET:
        n_old, identity, ts = -1, 0, None
    elif isinstance(old, tuple):
        n_old, identity, ts = old[1], 1, None
    else:
        n_old, identity, ts = len(old), 0, np.asarray(old, np.int64)
    a = None if act is None else np.ascontiguousarray(np.asarray(act, np.uint8))
    dense = np.full(max(n, 1), -99, np.int32)
    table = np.full(max(n_old, 0) + min(n, extent) + 1, -99, np.int64)
    n_new, status = C.c_int32(-1), C.c_uint32(99)
    _capi.check(_capi.lib().ibh_selftest_number_keys(
        stream.ctypes.data, keys.itemsize, stride, n, None if a is None else a.ctypes.data, extent, None if ts is None else ts.ctypes.data,
        n_old, identity, transform, check_range, dense.ctypes.data, table.ctypes.data, C.byref(n_new), C.byref(status)))
    assert table[max(n_old, 0) + max(n_new.value, 0)] == -99         # nothing past the table's end
    return dense[:n], (None if old is NO_SET else table[:n_old + n_new.value]), n_new.value, status.value


def reference(keys, extent, old=NO_SET, transform=ADD_DENSE, act=None, check_range=0):
    if old is NO_SET:
        table = list(range(extent))
    elif isinstance(old, tuple):
        table = list(range(old[1]))
    else:
        table = list(old)
    n_old = len(table)
    to_dense = {k: i for i, k in enumerate(table)}
    dense, status = [], 0
    for p, k in enumerate(int(k) for k in keys):
        if act is not None and not act[p]:
            dense.append(-1)
        elif k < 0 or k >= extent:
            assert check_range
            status |= OUT_OF_RANGE
            dense.append(-1)
        elif k in to_dense:
            dense.append(to_dense[k])
        elif transform == ADD_DENSE:
            to_dense[k] = len(table)
            table.append(k)
            dense.append(to_dense[k])
        else:
            status |= MISSING if transform == TO_DENSE else 0
            dense.append(-1)
    if status & OUT_OF_RANGE:           # a build fails there: the set stays as it was
        table = table[:n_old]
    return np.asarray(dense, np.int32), (None if old is NO_SET else np.asarray(table, np.int64)), len(table) - n_old, status


def check(keys, extent, **kw):
    dtype = kw.pop("dtype", np.int64)
    stride = kw.pop("stride", 1)
    got = run(keys, extent, stride=stride, dtype=dtype, **kw)
    ref = reference(keys, extent, **kw)
    assert np.array_equal(got[0], ref[0]), (kw, got[0], ref[0])
    assert (got[1] is None) == (ref[1] is None)
    if ref[1] is not None:
        assert np.array_equal(got[1], ref[1]), (kw, got[1], ref[1])
    assert got[2:] == ref[2:], (kw, got[2:], ref[2:])
    return got


WIDTHS = [np.int32, np.int64]
OLD_PARTS_7 = [NO_SET, [], ("identity", 0), ("identity", 3), ("identity", 7), [5, 2]]


@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 513])
def test_block_edges(n, dtype):
    """Stream lengths around the 256-thread blocks, over an extent the stream does not exhaust, against an empty set and a table."""
    extent = 300
    keys = np.random.default_rng(n).integers(0, extent, n)
    for old in ([], [299, 0, 17]):
        check(keys, extent, old=old, dtype=dtype)


@pytest.mark.parametrize("dtype", WIDTHS)
@pytest.mark.parametrize("old", OLD_PARTS_7, ids=lambda o: "none" if o is NO_SET else str(o).replace(" ", ""))
def test_old_parts_under_contention(old, dtype):
    """Extent 7, every key repeated many times over three blocks (atomicMin contended on one address per key), for every kind of old part."""
    keys = np.random.default_rng(7).integers(0, 7, 700)
    keys[:6] = [6, 6, 4, 2, 6, 0]
    check(keys, 7, old=old, dtype=dtype)
    check(np.full(600, 4), 7, old=old, dtype=dtype)


@pytest.mark.parametrize("dtype", WIDTHS)
def test_permutation(dtype):
    """No key repeats: every position is a first occurrence."""
    keys = np.random.default_rng(3).permutation(513)
    dense, table, n_new, status = check(keys, 513, old=[], dtype=dtype)
    assert n_new == 513 and status == 0 and np.array_equal(table, keys)
    check(keys, 513, old=("identity", 100), dtype=dtype)


@pytest.mark.parametrize("dtype", WIDTHS)
def test_act_masks_the_first_occurrence(dtype):
    """The first occurrence of key 5 is masked: its first ACTIVE occurrence is the one that is numbered, after key 3's."""
    keys = [5, 3, 5, 3, 5, 1]
    act = [0, 1, 1, 1, 1, 0]
    dense, table, n_new, status = check(keys, 8, old=[], act=act, dtype=dtype)
    assert table.tolist() == [3, 5] and dense.tolist() == [-1, 0, 1, 0, 1, -1]
    rng = np.random.default_rng(11)
    keys, act = rng.integers(0, 40, 600), rng.integers(0, 2, 600)
    for old in ([], [39, 7], ("identity", 5)):
        check(keys, 40, old=old, act=act, dtype=dtype)
    check(keys, 40, old=[39, 7], act=np.zeros(600, np.uint8), dtype=dtype)


@pytest.mark.parametrize("dtype", WIDTHS)
def test_stride_two(dtype):
    """The key of position p is keys[2 p], as the ice index (.y) of global_ec's exchange indices."""
    keys = np.random.default_rng(5).integers(0, 50, 300)
    for old in ([], [49, 3, 20]):
        check(keys, 50, old=old, stride=2, dtype=dtype)
    check(keys, 50, old=[], stride=2, act=np.arange(300) % 3 != 0, dtype=dtype)


@pytest.mark.parametrize("dtype", WIDTHS)
def test_to_dense_transforms(dtype):
    """TO_DENSE raises the status on a missing key, TO_DENSE_IGNORE_MISSING gives -1; neither grows the set."""
    keys = np.random.default_rng(9).integers(0, 10, 300)
    for old in ([5, 2], ("identity", 3), [], NO_SET, list(range(9, -1, -1))):
        for transform in (TO_DENSE, TO_DENSE_IGNORE_MISSING):
            dense, table, n_new, status = check(keys, 10, old=old, transform=transform, dtype=dtype)
            assert n_new == 0
    assert check(keys, 10, old=[5, 2], transform=TO_DENSE, dtype=dtype)[3] == MISSING
    dense, _, _, status = check(keys, 10, old=[5, 2], transform=TO_DENSE_IGNORE_MISSING, dtype=dtype)
    assert status == 0 and (dense == -1).sum() == ((keys != 5) & (keys != 2)).sum()
    assert check(keys, 10, old=NO_SET, transform=TO_DENSE, dtype=dtype)[3] == 0


@pytest.mark.parametrize("dtype", WIDTHS)
def test_keys_out_of_range(dtype):
    """Keys -1 and `extent` with the range check on: the status is raised, nothing is indexed with them (a table of `extent`
    entries and a first-occurrence table of `extent` words are all there is), the set stays as it was."""
    extent = 12
    keys = np.random.default_rng(13).integers(0, extent, 300)
    for bad in (-1, extent):
        k = keys.copy()
        k[[0, 17, 299]] = bad
        for old in ([], [5, 2], ("identity", 4)):
            for transform in (ADD_DENSE, TO_DENSE_IGNORE_MISSING):
                dense, table, n_new, status = check(k, extent, old=old, transform=transform, check_range=1, dtype=dtype)
                assert status == OUT_OF_RANGE and n_new == 0 and dense[[0, 17, 299]].tolist() == [-1, -1, -1]
    # the check on, nothing out of range: as without it
    assert check(keys, extent, old=[5, 2], check_range=1, dtype=dtype)[3] == 0
