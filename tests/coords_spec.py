"""Exact specifications of the coordinate, sort and dense-index kernels (csrc/coords.hip, csrc/sort.hip, the integer half of
csrc/dense.hip), in plain numpy and Python integers: dicts, sorted arrays and np.unique -- no hash table, nothing of oracle/coords.py.
Every integer output is specified exactly; the float outputs (es_interp_map weights, es_coords_to_points, the quotients inside the two
voxel-key kernels) are the same correctly rounded f32 operations in the same order (numpy's f32 +, -, *, / are correctly rounded),
compared bit for bit.  Nothing here has a tolerance.

PACKING AND DOMAIN.  key = b << 54 | (x + 2^17) << 36 | (y + 2^17) << 18 | (z + 2^17).  Coordinates lie in [LO, HI] = [-2^17, 2^17 - 1].
The largest sample index for which EVERY kernel is right is MAX_BATCH - 1 = 511, derived from the code:
  * the key must be non-negative: -1 is the empty table slot, and b << 54 < 2^63 needs b < 2^9;
  * k_batch_offsets / k_union_place recover b as `(int)(key >> 54)` with an ARITHMETIC shift: right for every non-negative key, i.e. the
    same b < 512 (a negative key would give a negative sample index);
  * k_morton forms `(uint64)b << 54 | 54 interleaved bits`: injective for b < 2^10, and the radix sort orders all 64 bits (8 passes of
    8 bits), so it is not the binding bound.  es_sort_u64 used to document keys < 2^62, which Morton keys of b >= 256 exceed; the
    header now says what the code does -- unsigned 64-bit order over all eight digits -- and the sort is specified and tested
    so: es_sort_u64 on keys with bit 62 and bit 63 set, es_morton_sort on samples up to b = 511.
n_batch <= MAX_BATCH and batch < MAX_BATCH; beyond that the entry points return -4.

EDGE OF THE FIELD.  A neighbour (es_kernel_map), interpolation corner (es_interp_map) or child (es_gen_children_keys) whose coordinate
falls outside [LO, HI] is ABSENT: -1 in the maps.  es_gen_children_keys writes rows 8 i + k positionally, so it cannot drop a row: the
absent child's row holds the absent key -1 (include/es_hip.h).  A neighbour is never another sample's voxel (a carry out of the x field)
and never a table fill value (the key -1 matching an empty slot).

VOXEL KEYS OUTSIDE THE DOMAIN.  q = p / vs (true f32 division), coordinate = trunc(q) toward zero for LO < q < HI; q >= HI gives HI,
q <= LO gives LO (saturation, +-inf included), NaN gives 0: every key written unpacks to its own sample index and to in-field
coordinates, and in-domain finite points are bit-exact with plain truncation.  es_voxel_keys_range: q = (p - min) / vs in f32, the same
quantisation, THEN the clamp to [0, cmax]; cmax is itself quantised into [0, HI].

TABLE CONTRACT.  cap is a power of two and greater than n; every entry point that takes a cap returns -4 on the host, before it touches
the device, when that does not hold (es_kernel_map / es_interp_map cannot know n: power of two only; es_union_plan: cap_a > na).  First
occurrence wins.  After es_unique_first the table maps each key to its unique row; after es_build_table to its row.  The table is checked
both as an array (check_table: every key once, value = row, all other slots empty) and through the device's own lookups (es_kernel_map
with ksize 1), which is where probing and the hash matter.

entry point            specification             cases (tests/test_gpu_coord_kernels.py; the emulator file runs the same bodies)
es_voxel_keys          voxel_keys                test_voxel_keys_around_every_boundary_and_outside_the_domain
es_voxel_keys_range    voxel_keys_range          test_voxel_keys_range_on_and_past_each_clamp_bound
es_unique_first        unique_first, check_table test_hash_table_*, test_scan_through_unique_first
es_build_table         build_table = rows, check_table, lookup   test_hash_table_*
es_stride_keys         stride_keys               test_stride_keys_and_interp_map_at_every_stride
es_keys_to_coords      keys_to_coords            test_keys_to_coords_and_points
es_coords_to_points    coords_to_points          test_keys_to_coords_and_points
es_batch_offsets       batch_offsets             test_batch_offsets_chain_and_union_over_sample_counts
es_strided_chain       strided_chain             test_batch_offsets_chain_and_union_over_sample_counts
es_gen_children_keys   gen_children              test_gen_children_keys_inside_and_at_the_end_of_the_field
es_kernel_map          kernel_map                test_kernel_and_inverse_maps_*, test_three_key_edge_of_the_field
es_inverse_map         inverse_map               test_kernel_and_inverse_maps_*
es_union_plan          union_plan                test_union_plan_*, test_scan_through_union_plan, test_batch_offsets_chain_and_union_...
es_interp_map          interp_map                test_stride_keys_and_interp_map_at_every_stride
es_compact_mask        compact_mask              test_scan_through_compact_mask
es_morton_sort         morton_sort (morton_key)  test_morton_sort_*
es_sort_u64            sort_u64                  test_sort_u64_*
es_sort_scratch_bytes  (the size every sort case passes exactly; one byte less returns -5)
es_volume_map          volume_map                test_dense_maps
es_volume_up_index     volume_up_index           test_dense_maps
es_dense_index         dense_index               test_dense_maps
"""
import numpy as np

FIELD = 18
OFF = 1 << 17
LO, HI = -OFF, OFF - 1
FMASK = (1 << FIELD) - 1
MAX_BATCH = 512
ABSENT_KEY = -1
F32 = np.float32
I64 = np.int64


# ------------------------------------------------------------------------------------------------------------------ keys
def pack(b, x, y, z):
    """(arrays of) in-field coordinates -> int64 keys"""
    b, x, y, z = (np.asarray(v, dtype=I64) for v in (b, x, y, z))
    assert np.all((b >= 0) & (b < MAX_BATCH)) and np.all(in_field(x, y, z)), 'pack() is defined on the domain only'
    return (b << 54) | ((x + OFF) << 36) | ((y + OFF) << 18) | (z + OFF)


def unpack(keys):
    k = np.asarray(keys, dtype=I64)
    return k >> 54, ((k >> 36) & FMASK) - OFF, ((k >> 18) & FMASK) - OFF, (k & FMASK) - OFF


def in_field(x, y, z):
    x, y, z = (np.asarray(v, dtype=I64) for v in (x, y, z))
    return (x >= LO) & (x <= HI) & (y >= LO) & (y <= HI) & (z >= LO) & (z <= HI)


def rows_of(keys):
    """{key: row} of a unique key list (a dict: the specification's table)"""
    d = {int(k): i for i, k in enumerate(np.asarray(keys).tolist())}
    assert len(d) == len(keys), 'rows_of() wants unique keys'
    return d


def lookup(in_keys, q, valid=None):
    """row of each query key in the unique list in_keys, -1 when absent or not `valid` (sorted array + binary search)"""
    in_keys, q = np.asarray(in_keys, dtype=I64), np.asarray(q, dtype=I64)
    out = np.full(q.shape, -1, dtype=np.int32)
    if in_keys.size == 0 or q.size == 0:
        return out
    order = np.argsort(in_keys, kind='stable')
    sk = in_keys[order]
    assert np.all(sk[1:] != sk[:-1]), 'lookup() wants unique keys'
    pos = np.minimum(np.searchsorted(sk, q), sk.size - 1)
    hit = sk[pos] == q
    if valid is not None:
        hit &= valid
    return np.where(hit, order[pos], -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ voxel keys
def quant(q):
    """f32 quotients -> coordinates: truncation inside the field, saturation beyond it, NaN -> 0"""
    q = np.asarray(q, dtype=F32)
    out = np.zeros(q.shape, dtype=I64)
    nan = np.isnan(q)
    hi, lo = ~nan & (q >= F32(HI)), ~nan & (q <= F32(LO))
    mid = ~(nan | hi | lo)
    out[mid] = np.trunc(q[mid]).astype(I64)
    out[hi], out[lo] = HI, LO
    return out


def voxel_keys(points, batch, vs):
    """points: (n, ld >= 3) f32"""
    p = np.asarray(points, dtype=F32)[:, :3]
    with np.errstate(all='ignore'):
        c = quant(p / F32(vs))
    return pack(np.full(len(p), batch), c[:, 0], c[:, 1], c[:, 2])


def voxel_keys_range(points, batch, rng):
    """rng: 9 f32 {min xyz, voxel size xyz, clamp max xyz}: subtract, divide, truncate (quant), clamp to [0, quant(cmax)]"""
    p = np.asarray(points, dtype=F32)[:, :3]
    rng = np.asarray(rng, dtype=F32)
    with np.errstate(all='ignore'):
        c = quant((p - rng[None, 0:3]) / rng[None, 3:6])
    cmax = np.maximum(quant(rng[6:9]), 0)
    c = np.minimum(np.maximum(c, 0), cmax[None])
    return pack(np.full(len(p), batch), c[:, 0], c[:, 1], c[:, 2])


# ------------------------------------------------------------------------------------------------------------------ unique / table
def unique_first(keys):
    """-> (out_keys, out_src): the distinct keys in order of their FIRST occurrence, and that occurrence's index"""
    keys = np.asarray(keys, dtype=I64)
    if keys.size == 0:
        return keys.copy(), np.zeros(0, dtype=np.int32)
    _, first = np.unique(keys, return_index=True)
    src = np.sort(first)
    return keys[src], src.astype(np.int32)


def check_table(label, tkeys, tvals, unique_keys, fill):
    """the (tkeys, tvals) arrays hold every key of unique_keys exactly once with its row; every other slot is empty (key -1, value
    `fill`).  Independent of the hash and of the probing order."""
    tkeys, tvals, uk = np.asarray(tkeys), np.asarray(tvals), np.asarray(unique_keys, dtype=I64)
    used = tkeys != ABSENT_KEY
    gk, gv = tkeys[used], tvals[used]
    assert len(gk) == len(uk), f'{label}: the table holds {len(gk)} keys, the set has {len(uk)}'
    o_got, o_want = np.argsort(gk, kind='stable'), np.argsort(uk, kind='stable')          # sorted arrays: row of key uk[o_want[i]] is o_want[i]
    assert np.all(np.diff(uk[o_want]) != 0), 'check_table() wants unique keys'
    assert np.all(np.diff(gk[o_got]) != 0), f'{label}: a key sits in two slots'
    assert np.array_equal(gk[o_got], uk[o_want]), f'{label}: the keys in the table are not the keys of the set'
    assert np.array_equal(gv[o_got], o_want), f'{label}: the table does not map each key to its row'
    assert np.all(tvals[~used] == fill), f'{label}: an empty slot carries a value other than the fill {fill}'


# ------------------------------------------------------------------------------------------------------------------ key transforms
def stride_keys(keys, ts):
    b, x, y, z = unpack(keys)
    return pack(b, x // ts * ts, y // ts * ts, z // ts * ts)           # numpy // on integers is the true floor


def keys_to_coords(keys):
    return np.stack(unpack(keys), 1).astype(np.int32)


def coords_to_points(coords, vs):
    return np.asarray(coords)[:, 1:].astype(F32) * F32(vs)


def batch_offsets(keys, n_batch):
    """offsets[b] = first row with sample index >= b, b = 0 .. n_batch (rows batch-major)"""
    b = np.asarray(keys, dtype=I64) >> 54
    assert np.all(b[1:] >= b[:-1]), 'batch_offsets() wants batch-major rows'
    return np.searchsorted(b, np.arange(n_batch + 1), side='left').astype(np.int32)


def strided_chain(root_keys, n_batch, ts_list):
    """-> ([out_keys of level l], res): every level is the first-occurrence unique of the ROOT keys floored to ts[l];
    res = per level [count, offsets[0 .. n_batch]]"""
    levels, res = [], []
    for ts in ts_list:
        ok, _ = unique_first(stride_keys(root_keys, ts))
        levels.append(ok)
        res.append(np.concatenate([[len(ok)], batch_offsets(ok, n_batch)]))
    return levels, np.concatenate(res).astype(np.int32) if res else np.zeros(0, dtype=np.int32)


def gen_children(keys, half):
    """row 8 i + k = parent i + half * (k & 1, k >> 1 & 1, k >> 2 & 1); the absent key where that leaves the field"""
    b, x, y, z = unpack(keys)
    k = np.arange(8)
    cx, cy, cz = x[:, None] + (k & 1) * half, y[:, None] + ((k >> 1) & 1) * half, z[:, None] + ((k >> 2) & 1) * half
    ok = in_field(cx, cy, cz)
    out = np.full(cx.shape, ABSENT_KEY, dtype=I64)
    bb = np.broadcast_to(b[:, None], cx.shape)
    out[ok] = pack(bb[ok], cx[ok], cy[ok], cz[ok])
    return out.reshape(-1)


# ------------------------------------------------------------------------------------------------------------------ maps
def kernel_offsets(ksize, in_ts):
    """(K, 3) offsets, x fastest; centred for odd kernels, 0 .. ksize - 1 for even ones"""
    c = ksize // 2 if ksize % 2 else 0
    k = np.arange(ksize ** 3)
    return np.stack([(k % ksize - c), ((k // ksize) % ksize - c), (k // (ksize * ksize) - c)], 1) * in_ts


def kernel_map(out_keys, in_keys, ksize, in_ts):
    """nbr (n_out, K): row of in_keys (unique; row = position) at out_j + offset_k, -1 if none or outside the field"""
    b, x, y, z = unpack(out_keys)
    o = kernel_offsets(ksize, in_ts)
    nx, ny, nz = x[:, None] + o[None, :, 0], y[:, None] + o[None, :, 1], z[:, None] + o[None, :, 2]
    ok = in_field(nx, ny, nz)
    q = np.zeros(nx.shape, dtype=I64)
    bb = np.broadcast_to(b[:, None], nx.shape)
    q[ok] = pack(bb[ok], nx[ok], ny[ok], nz[ok])
    return lookup(in_keys, q, ok)


def inverse_map(nbr, n_in):
    """inv (n_in, K): inv[i][k] = j where nbr[j][k] == i, else -1"""
    nbr = np.asarray(nbr)
    K = nbr.shape[1] if nbr.ndim == 2 else 1
    inv = np.full((n_in, K), -1, dtype=np.int32)
    j, k = np.nonzero(nbr >= 0)
    i = nbr[j, k]
    assert len(set(zip(i.tolist(), k.tolist()))) == len(i), 'two output rows claim one (input row, tap)'
    inv[i, k] = j
    return inv


def union_plan(keys_a, keys_b, n_batch):
    """sparse a + b: out rows batch-major, inside a sample a's rows (in a's order) then b's new rows (in b's order).
    -> (pos_a, pos_b, out_keys, count)"""
    ka, kb = np.asarray(keys_a, dtype=I64), np.asarray(keys_b, dtype=I64)
    hit = lookup(ka, kb)
    new = hit < 0
    allk = np.concatenate([ka, kb[new]])
    side = np.concatenate([np.zeros(len(ka), dtype=I64), np.ones(int(new.sum()), dtype=I64)])
    idx = np.concatenate([np.arange(len(ka)), np.arange(int(new.sum()))])
    order = np.lexsort((idx, side, allk >> 54))
    place = np.empty(len(allk), dtype=np.int32)
    place[order] = np.arange(len(allk), dtype=np.int32)
    pos_a = place[:len(ka)]
    pos_b = np.empty(len(kb), dtype=np.int32)
    pos_b[new] = place[len(ka):]
    pos_b[~new] = pos_a[hit[~new]]
    return pos_a, pos_b, allk[order], len(allk)


def interp_map(q_keys, table_keys, ts):
    """idx (n, 8), w (n, 8): the 8 corners lo + ts * (k & 1, k >> 1 & 1, k >> 2 & 1) of the query's cell in the stride-ts set and the
    trilinear weights, f32: f = f32(c - lo) / f32(ts); w = ((1 * wx) * wy) * wz with w? = f or (1 - f)"""
    b, x, y, z = unpack(q_keys)
    lo = [v // ts * ts for v in (x, y, z)]
    f = [(v - l).astype(F32) / F32(ts) for v, l in zip((x, y, z), lo)]
    k = np.arange(8)
    s = [(k & 1), (k >> 1) & 1, (k >> 2) & 1]
    c = [l[:, None] + sk[None] * ts for l, sk in zip(lo, s)]
    ok = in_field(*c)
    q = np.zeros(c[0].shape, dtype=I64)
    bb = np.broadcast_to(b[:, None], q.shape)
    q[ok] = pack(bb[ok], c[0][ok], c[1][ok], c[2][ok])
    w = np.ones(q.shape, dtype=F32)
    for fa, sk in zip(f, s):
        w = w * np.where(sk[None] == 1, fa[:, None], F32(1) - fa[:, None]).astype(F32)
    return lookup(table_keys, q, ok), w.astype(F32)


def compact_mask(keys, mask):
    src = np.nonzero(np.asarray(mask) != 0)[0].astype(np.int32)
    return np.asarray(keys)[src], src


# ------------------------------------------------------------------------------------------------------------------ sort
def morton_key(b, x, y, z):
    """Python integers: bit i of (z + 2^17) -> bit 3 i, of (y + 2^17) -> 3 i + 1, of (x + 2^17) -> 3 i + 2; sample above bit 54"""
    ux, uy, uz = int(x) + OFF, int(y) + OFF, int(z) + OFF
    m = 0
    for i in range(FIELD):
        m |= ((uz >> i) & 1) << (3 * i) | ((uy >> i) & 1) << (3 * i + 1) | ((ux >> i) & 1) << (3 * i + 2)
    return (int(b) << 54) | m


def morton_keys(keys):
    """the same interleave on arrays (uint64); test_emu_coord_kernels checks it against morton_key"""
    b, x, y, z = (v.astype(np.uint64) for v in unpack(keys))
    off, one = np.uint64(OFF), np.uint64(1)
    m = np.zeros(len(b), dtype=np.uint64)
    for i in range(FIELD):
        for a, v in enumerate((z, y, x)):
            m |= (((v + off) >> np.uint64(i)) & one) << np.uint64(3 * i + a)
    return (b << np.uint64(54)) | m


def _sorted_by(order_keys, keys, src):
    order = np.argsort(order_keys, kind='stable')
    return np.asarray(keys)[order], (None if src is None else np.asarray(src)[order])


def morton_sort(keys, src):
    """(out_keys, out_src): rows in ascending Morton-key order, ties (equal keys) in input order"""
    return _sorted_by(morton_keys(keys), keys, src)


def sort_u64(keys, src):
    """ascending, stable, keys read as unsigned 64-bit"""
    return _sorted_by(np.asarray(keys, dtype=I64).view(np.uint64), keys, src)


# ------------------------------------------------------------------------------------------------------------------ dense
def volume_map(B, X, Y, Z, Xo, Yo, Zo, ks, stride, pad):
    """nbr (B Xo Yo Zo, ks^3): row ((b X + x) Y + y) Z + z of the tap, tap = (kx ks + ky) ks + kz, -1 outside the grid"""
    b, xo, yo, zo, kx, ky, kz = np.meshgrid(*(np.arange(v) for v in (B, Xo, Yo, Zo, ks, ks, ks)), indexing='ij')
    x, y, z = xo * stride - pad + kx, yo * stride - pad + ky, zo * stride - pad + kz
    ok = (x >= 0) & (x < X) & (y >= 0) & (y < Y) & (z >= 0) & (z < Z)
    return np.where(ok, ((b * X + x) * Y + y) * Z + z, -1).astype(np.int32).reshape(B * Xo * Yo * Zo, ks ** 3)


def volume_up_index(B, X, Y, Z):
    """idx (B 2X 2Y 2Z): 8 * (row of the parent voxel) + ((xo & 1) 2 + (yo & 1)) 2 + (zo & 1)"""
    b, xo, yo, zo = np.meshgrid(*(np.arange(v) for v in (B, 2 * X, 2 * Y, 2 * Z)), indexing='ij')
    i = ((b * X + xo // 2) * Y + yo // 2) * Z + zo // 2
    return (i * 8 + ((xo & 1) * 2 + (yo & 1)) * 2 + (zo & 1)).astype(np.int32).reshape(-1)


def dense_index(coords, ts, X, Y, Z):
    """idx[i] = ((b X + x / ts) Y + y / ts) Z + z / ts, -1 for a negative coordinate or one past a face"""
    c = np.asarray(coords, dtype=I64)
    b, x, y, z = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    ok = (x >= 0) & (y >= 0) & (z >= 0) & (x // ts < X) & (y // ts < Y) & (z // ts < Z)
    return np.where(ok, ((b * X + x // ts) * Y + y // ts) * Z + z // ts, -1).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------ comparison
def same(label, got, want):
    """every element equal (floats: bit for bit)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f'{label}: shape {got.shape}, specified {want.shape}'
    if got.dtype.kind == 'f':
        assert want.dtype == got.dtype
        got, want = got.view(np.uint32), want.view(np.uint32)
    bad = np.nonzero(got.reshape(-1) != want.reshape(-1))[0]
    assert bad.size == 0, (f'{label}: {bad.size} of {got.size} elements differ, first at {int(bad[0])}: '
                           f'{got.reshape(-1)[bad[0]]} != specified {want.reshape(-1)[bad[0]]}')
