"""CPU: the two functions that hand the matrix-core filter's work units to its waves (ivf_pq_filter_common.hpp: unit_cost_key,
unit_share_len / unit_position), through the exported hook - pq_filter4_kernel, pq_filter_kernel and order_units_kernel call the
same functions on the device."""
import ctypes as C


def hook(rows=0, groups=1, unit_rows=8192, n_units=0, xcd=0, t=0, strided=1):
    from cuvs_amd._lib import lib

    fn = lib().cuvsAmdIvfPqUnitOrderHook
    fn.argtypes = [C.c_uint32] * 6 + [C.c_int, C.c_void_p]
    fn.restype = None
    out = (C.c_uint32 * 3)()
    fn(rows, groups, unit_rows, n_units, xcd, t, strided, C.addressof(out))
    return int(out[0]), int(out[1]), int(out[2])


def test_every_position_is_handed_out_exactly_once():
    """n_units = 0 .. 70: the pairs (xcd, t < share_len(xcd)) map onto every position exactly once - in the strided shares of
    the cost order and in the contiguous shares of the list order."""
    for strided in (1, 0):
        for n in range(71):
            seen = []
            for xcd in range(8):
                share_len = hook(n_units=n, xcd=xcd, strided=strided)[1]
                seen += [hook(n_units=n, xcd=xcd, t=t, strided=strided)[2] for t in range(share_len)]
            assert sorted(seen) == list(range(n)), (strided, n, seen)


def test_strided_shares_interleave():
    """ticket t of XCD x is position 8 t + x: every share walks the whole array, so it ends on the array's cheap end"""
    for n in (1, 7, 8, 9, 70):
        for xcd in range(8):
            assert hook(n_units=n, xcd=xcd)[1] == (n - xcd + 7) // 8
            assert hook(n_units=n, xcd=xcd, t=3)[2] == 24 + xcd


def test_cost_key_is_monotone_and_zero_rows_come_last():
    for unit_rows in (4096, 8192, 20032):
        keys = [[hook(rows=r, groups=g, unit_rows=unit_rows)[0] for r in range(0, unit_rows + 1, 32)] for g in (1, 2, 3, 4)]
        for g in range(4):
            assert keys[g][0] == 0, "a unit without rows has the key that is placed last"
            assert all(a <= b for a, b in zip(keys[g], keys[g][1:])), "non-decreasing in rows"
            assert min(keys[g][1:]) >= 1 and max(keys[g]) <= 511
        for g in range(3):
            assert all(a <= b for a, b in zip(keys[g], keys[g + 1])), "non-decreasing in the group count"
        assert keys[3][-1] > keys[0][-1] > keys[0][1], "the keys tell costs apart"
    # rows between two multiples of 32 cost the subtile they start
    assert hook(rows=1, groups=1)[0] == hook(rows=32, groups=1)[0] <= hook(rows=33, groups=1)[0]
    # beyond the chunk length and beyond four groups the key stays in range
    assert hook(rows=10 ** 6, groups=9, unit_rows=8192)[0] == 511
