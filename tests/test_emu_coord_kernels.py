"""tests/test_gpu_coord_kernels.py on the CPU emulator (tests/emu): the same bodies on the same shapes, under the `emulated` fixture of
tests/test_emu_product.py (random thread schedule); the hash table, the union, the offset search and the sort also under the `descending`
and another seeded `random` schedule.  Then the specification itself: it alone handles every size of the grids (no kernel involved),
its Python-integer Morton interleave agrees with the array form, it agrees with oracle/coords.py on a small cloud, and it rejects a
correct output with ONE thing wrong.
TEST INFRASTRUCTURE: the product binds libes_hip.so only."""
import ctypes

import numpy as np
import pytest

import coords_spec as S
import test_gpu_coord_kernels as T
from test_emu_product import emulated  # noqa: F401  (the fixture that puts the product's host layer on the emulator)

CPU = __import__('torch').device('cpu')


def _schedule(order, seed=4242):
    import build as emu_build
    lib = ctypes.CDLL(emu_build.build())
    lib.es_emu_set_schedule.argtypes = [ctypes.c_int, ctypes.c_ulonglong]
    lib.es_emu_set_schedule(order, seed)


# ------------------------------------------------------------------------------------------------------------ the GPU bodies
@pytest.mark.parametrize('kind', ['wrap', 'equal', 'distinct', 'dups'])
def test_hash_table_at_every_load(emulated, kind):  # noqa: F811
    T.test_hash_table_at_every_load(emulated, kind)


def test_hash_table_refuses_a_bad_capacity(emulated):  # noqa: F811
    T.test_hash_table_refuses_a_bad_capacity(emulated)


@pytest.mark.parametrize('n', T.SCAN_NS)
def test_scan_through_compact_mask(emulated, n):  # noqa: F811
    T.test_scan_through_compact_mask(emulated, n)


@pytest.mark.parametrize('n', T.SCAN_NS)
def test_scan_through_unique_first(emulated, n):  # noqa: F811
    T.test_scan_through_unique_first(emulated, n)


@pytest.mark.parametrize('n', T.SCAN_NS)
def test_scan_through_union_plan(emulated, n):  # noqa: F811
    T.test_scan_through_union_plan(emulated, n)


def test_union_plan_with_empty_nested_disjoint_and_one_sided_operands(emulated):  # noqa: F811
    T.test_union_plan_with_empty_nested_disjoint_and_one_sided_operands(emulated)


@pytest.mark.parametrize('n_batch', T.N_BATCHES)
def test_batch_offsets_chain_and_union_over_sample_counts(emulated, n_batch):  # noqa: F811
    T.test_batch_offsets_chain_and_union_over_sample_counts(emulated, n_batch)


def test_sample_counts_above_the_maximum_are_refused(emulated):  # noqa: F811
    T.test_sample_counts_above_the_maximum_are_refused(emulated)


@pytest.mark.parametrize('in_ts', [1, 2, 8, 64])
def test_kernel_and_inverse_maps(emulated, in_ts):  # noqa: F811
    T.test_kernel_and_inverse_maps_on_the_kernel_and_stride_grid(emulated, in_ts)
    if in_ts == 1:
        T.test_kernel_and_inverse_maps_with_empty_operands(emulated)


@pytest.mark.parametrize('via_unique', [False, True])
def test_three_key_edge_of_the_field(emulated, via_unique):  # noqa: F811
    T.test_three_key_edge_of_the_field(emulated, via_unique)


@pytest.mark.parametrize('ts', [2, 4, 8, 16, 32, 64])
def test_stride_keys_and_interp_map_at_every_stride(emulated, ts):  # noqa: F811
    T.test_stride_keys_and_interp_map_at_every_stride(emulated, ts)


def test_children_coords_and_points(emulated):  # noqa: F811
    T.test_gen_children_keys_inside_and_at_the_end_of_the_field(emulated)
    T.test_keys_to_coords_and_points(emulated)


@pytest.mark.parametrize('n', T.SORT_NS)
def test_sort_u64_on_the_size_grid(emulated, n):  # noqa: F811
    T.test_sort_u64_on_the_size_grid(emulated, n)


@pytest.mark.parametrize('n', [257, 2049, 32769])
def test_sort_u64_pass_patterns_and_both_result_parities(emulated, n):  # noqa: F811
    T.test_sort_u64_pass_patterns_and_both_result_parities(emulated, n)


@pytest.mark.parametrize('n', [1, 2, 257, 2049, 32769])
def test_morton_sort_over_the_whole_field_and_sample_range(emulated, n):  # noqa: F811
    T.test_morton_sort_over_the_whole_field_and_sample_range(emulated, n)


@pytest.mark.parametrize('vs', [0.01, 0.02, 0.16])
def test_voxel_keys_around_every_boundary_and_outside_the_domain(emulated, vs):  # noqa: F811
    T.test_voxel_keys_around_every_boundary_and_outside_the_domain(emulated, vs)


def test_voxel_keys_range_on_and_past_each_clamp_bound(emulated):  # noqa: F811
    T.test_voxel_keys_range_on_and_past_each_clamp_bound(emulated)


def test_dense_maps(emulated):  # noqa: F811
    T.test_dense_maps(emulated)


# ------------------------------------------------------------------------------------------------------------ other thread schedules
@pytest.mark.parametrize('order,seed', [(0, 1), (1, 1), (2, 99)])
def test_tables_unions_offsets_and_sorts_under_other_schedules(emulated, order, seed):  # noqa: F811
    """schedule 0 / 1: ascending / descending thread order between synchronisation points; 2: random with another seed"""
    _schedule(order, seed)
    T.table_case(emulated, 1023, 'least', 'wrap', 5, True)
    T.table_case(emulated, 1024, 'least', 'equal', 6, False)
    T.table_case(emulated, 300, 'product', 'dups', 7, True)
    T.compact_case(emulated, 2049, 'random', 8)
    T.test_batch_offsets_chain_and_union_over_sample_counts(emulated, 300)
    T.test_three_key_edge_of_the_field(emulated, True)
    T.test_sort_u64_on_the_size_grid(emulated, 2049)
    T.test_morton_sort_over_the_whole_field_and_sample_range(emulated, 257)


# ------------------------------------------------------------------------------------------------------------ the specification alone
def _rejected(fn, what):
    try:
        fn()
    except AssertionError:
        return
    raise AssertionError(f'the specification accepted {what}')


def test_specification_alone_handles_every_size_of_the_grids():
    """no kernel: at every n of the scan, sort, table and sample-count grids the numpy specification produces a full-length output whose
    defining properties hold when checked another way (Python dict / set / sorted())"""
    for n in T.SCAN_NS:
        rng = T._rng(n)
        keys = T.scan_unique_keys(rng, n, 'random')
        uk, src = S.unique_first(keys)
        assert len(set(uk.tolist())) == len(uk) == len(set(keys.tolist())) and np.all(keys[src] == uk) and np.all(np.diff(src) > 0)
        seen = np.zeros(n, dtype=bool)
        seen[src] = True
        assert np.all(src[S.lookup(uk, keys[~seen])] < np.nonzero(~seen)[0]), 'a later occurrence precedes the chosen one'
        mask = T._flags(rng, n, 'random')
        ck, cs = S.compact_mask(keys, mask)
        assert len(ck) == int(mask.sum()) and np.all(mask[cs] == 1) and np.all(np.diff(cs) > 0) and np.all(ck == keys[cs])
        ka, kb = T.union_sets(rng, n, 'random')
        pa, pb, ok, cnt = S.union_plan(ka, kb, 3)
        assert cnt == len(set(ka.tolist()) | set(kb.tolist())) == len(ok) and np.all(ok[pa] == ka) and np.all(ok[pb] == kb)
        assert np.all(np.diff(ok >> 54) >= 0) and len(set(ok.tolist())) == cnt
    for n in T.SORT_NS:
        rng = T._rng(n)
        for pattern in ('bit61', 'dups'):
            keys, src = T.sort_keys(rng, n, pattern), np.arange(n, dtype=np.int32)[::-1].copy()
            sk, ss = S.sort_u64(keys, src)
            assert len(sk) == n and np.all(np.diff(sk) >= 0) and np.all(keys[n - 1 - ss] == sk)
            tie = np.diff(sk) == 0
            assert np.all(np.diff(ss)[tie] < 0), 'equal keys keep their input order (the payload is reversed)'
    for n, _ in T.TABLE_LOADS:
        for keys in (T.keys_hashing_to_last_slot(T._rng(n), n, T._cap_for(n)), T.distinct_keys(T._rng(n), n)):
            rows = np.arange(n, dtype=np.int32)
            assert len(keys) == n and np.all(keys >= 0) and len(set(keys.tolist())) == n
            perm = T._rng(n + 1).permutation(n)
            assert np.array_equal(S.lookup(keys, keys[perm]), rows[perm]) and np.all(S.lookup(keys, T.absent_keys(T._rng(n), keys, n)) == -1)
            assert [S.rows_of(keys)[int(k)] for k in keys[perm]] == perm.tolist()
            uk, src = S.unique_first(np.concatenate([keys, keys[perm]]))
            assert np.array_equal(uk, keys) and np.array_equal(src, rows)
    for nb in T.N_BATCHES + [S.MAX_BATCH + 1]:
        keys = T.random_set(T._rng(nb), 3 * nb + 40, min(nb, S.MAX_BATCH), empty=T.sample_layout(nb))
        off = S.batch_offsets(keys, nb)
        b = (keys >> 54).tolist()
        assert len(off) == nb + 1 and [int(v) for v in off] == [sum(1 for t in b if t < s) for s in range(nb + 1)]


def test_morton_interleave_in_python_integers_is_the_array_form():
    rng = T._rng(4)
    keys = T.morton_inputs(rng, 600)
    b, x, y, z = S.unpack(keys)
    py = [S.morton_key(*t) for t in zip(b.tolist(), x.tolist(), y.tolist(), z.tolist())]
    assert py == S.morton_keys(keys).tolist()
    assert S.morton_key(0, S.LO, S.LO, S.LO) == 0 and S.morton_key(511, S.HI, S.HI, S.HI) == (1 << 63) - 1
    assert S.morton_key(0, S.LO, S.LO, S.LO + 1) == 1 and S.morton_key(0, S.LO, S.LO + 1, S.LO) == 2 and S.morton_key(0, S.LO + 1, S.LO, S.LO) == 4
    order = sorted(range(len(py)), key=lambda i: py[i])
    assert np.array_equal(S.morton_sort(keys, None)[0], keys[order])


def test_specification_agrees_with_the_oracle_on_a_small_cloud():
    """the ONE cross-check against oracle/coords.py (the specification does not import it)"""
    from oracle import coords as C
    rng = T._rng(12)
    pts = [((rng.random((n, 3)) * 4 - 2).astype(np.float32)) for n in (400, 1, 250)]
    oc, osrc = C.voxelize(pts, 0.16)
    keys = np.concatenate([S.voxel_keys(p, b, 0.16) for b, p in enumerate(pts)])
    uk, src = S.morton_sort(*S.unique_first(keys))                              # (the oracle's root set is laid out along the Z-curve)
    assert np.array_equal(S.keys_to_coords(uk), oc) and np.array_equal(src.astype(np.int64), osrc)
    o2 = C.stride_coords(oc, 2)
    s2, _ = S.unique_first(S.stride_keys(uk, 2))
    assert np.array_equal(S.keys_to_coords(s2), o2)
    for ks in (2, 3):
        onbr = C.kernel_map(oc, o2, ks, 1)
        nbr = S.kernel_map(s2, uk, ks, 1)
        assert np.array_equal(nbr, onbr) and np.array_equal(S.inverse_map(nbr, len(uk)), C.inverse_map(onbr, len(uk)))
    och = C.gen_transpose_coords(o2, 2)
    ch = S.gen_children(s2, 1)
    assert np.array_equal(S.keys_to_coords(ch), och)
    ou, opa, opb = C.union_coords(oc, och, 3)
    pa, pb, ok, cnt = S.union_plan(uk, ch, 3)
    assert np.array_equal(S.keys_to_coords(ok), ou) and np.array_equal(pa, opa) and np.array_equal(pb, opb)


def test_specification_rejects_one_thing_wrong():
    """two rows swapped; a second occurrence instead of the first; one neighbour off by one row; one offset short; an unstable tie; a
    table value off by one row; a weight one ulp off; a neighbour in another sample; a fill value for a neighbour"""
    rng = T._rng(2)
    base = T.distinct_keys(rng, 40)
    keys = base[rng.integers(0, 40, size=200)]
    uk, src = S.unique_first(keys)
    S.same('good', uk, S.unique_first(keys)[0])
    sw = uk.copy()
    sw[[3, 4]] = sw[[4, 3]]
    _rejected(lambda: S.same('swapped', sw, uk), 'two rows swapped')
    second = src.copy()
    dup = next(i for i in range(len(uk)) if int((keys == uk[i]).sum()) > 1)
    second[dup] = np.nonzero(keys == uk[dup])[0][1]
    assert keys[second[dup]] == uk[dup]
    _rejected(lambda: S.same('second', second, src), 'a second occurrence chosen instead of the first')
    cap = 256
    tk, tv = np.full(cap, -1, dtype=np.int64), np.full(cap, T.FILL_UNIQUE, dtype=np.int32)
    tk[:len(uk)], tv[:len(uk)] = uk, np.arange(len(uk))
    S.check_table('good', tk, tv, uk, T.FILL_UNIQUE)
    bad = tv.copy()
    bad[5] += 1
    _rejected(lambda: S.check_table('row', tk, bad, uk, T.FILL_UNIQUE), 'a table value off by one row')
    bad = tv.copy()
    bad[cap - 1] = 0
    _rejected(lambda: S.check_table('fill', tk, bad, uk, T.FILL_UNIQUE), 'a value in an empty slot')
    twice = tk.copy()
    twice[cap - 1] = uk[0]
    _rejected(lambda: S.check_table('twice', twice, tv, uk, T.FILL_UNIQUE), 'a key in two slots')
    ins = T.random_set(rng, 300, 2, span=4)
    nbr = S.kernel_map(ins, ins, 3, 1)
    off1 = nbr.copy()
    j, k = np.argwhere(nbr >= 0)[7]
    off1[j, k] += 1
    _rejected(lambda: S.same('nbr', off1, nbr), 'one neighbour off by one row')
    offs = S.batch_offsets(ins, 2)
    short = offs.copy()
    short[1] -= 1
    _rejected(lambda: S.same('offsets', short, offs), 'one offset short')
    sk = T.sort_keys(rng, 500, 'dups')
    rev = np.arange(500, dtype=np.int32)[::-1].copy()
    wk, ws = S.sort_u64(sk, rev)
    t = int(np.nonzero(np.diff(wk) == 0)[0][0])
    unstable = ws.copy()
    unstable[[t, t + 1]] = unstable[[t + 1, t]]
    assert np.array_equal(sk[499 - unstable], wk)                                # still a correct sort of the keys
    _rejected(lambda: S.same('tie', unstable, ws), 'an unstable tie')
    # the two defects of the field's edge, as outputs: a neighbour in another sample; the fill value of an empty slot
    ek = T.edge_keys()
    ek = ek[np.argsort(ek >> 54, kind='stable')]
    good = S.kernel_map(ek, ek, 3, 1)
    row = {int(k): i for i, k in enumerate(ek)}
    other = good.copy()
    other[row[int(S.pack(0, S.HI, 0, 0))], 14] = row[int(S.pack(1, S.LO, 0, 0))]
    _rejected(lambda: S.same('sample', other, good), 'a neighbour in another sample')
    fill = good.copy()
    fill[row[int(S.pack(0, 0, 0, S.LO))], :9] = T.FILL_UNIQUE
    _rejected(lambda: S.same('fill', fill, good), 'a table fill value as a neighbour')
    q = S.pack([0, 0], [3, -5], [1, 7], [2, 0])
    idx, w = S.interp_map(q, S.stride_keys(q, 4), 4)
    w2 = w.copy()
    w2[0, 0] = np.nextafter(w2[0, 0], np.float32(2))
    _rejected(lambda: S.same('weights', w2, w), 'a weight one ulp off')
    assert np.all(w.astype(np.float64).sum(1) == 1.0) and int((idx >= 0).sum()) >= 2
