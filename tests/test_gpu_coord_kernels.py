"""The coordinate, sort and dense-index kernels (csrc/coords.hip, csrc/sort.hip, the integer half of csrc/dense.hip) held to the exact
specifications of tests/coords_spec.py, through the C ABI itself (not embodiedscan_amd/sparse.py): table capacities down to the smallest
legal one, scratch buffers of exactly the documented size, the shapes at which each mechanism changes path (SCAN_B = 2048 and the
256-block carry loop of the scan, the 4096-entry slab and the 1024-workgroup stride of the radix sort, the one-workgroup offset search,
the grid strides of the dense maps) and the edge of the 18-bit coordinate field.  Every output and scratch buffer sits between two
sentinel pads that must survive; every element of every output is compared.

Every body is a function of `dev`: tests/test_emu_coord_kernels.py runs the same bodies on the CPU emulator."""
import ctypes

import numpy as np
import pytest
import torch

import coords_spec as S
from test_gpu_ground_kernels import _hip, _rc, _st

pytestmark = pytest.mark.gpu

PAD = 16
SENT = {torch.int32: -77, torch.int64: -7777777777, torch.float32: -777.25, torch.uint8: 0xA5}
FILL_UNIQUE, FILL_BUILD = 0x7F7F7F7F, -1


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda:0')


class Buf:
    """n elements between two pads of PAD sentinels (the body too starts as sentinels)"""

    def __init__(self, dev, n, dtype=torch.int32, pad=PAD):
        self.n, self.pad, self.sent = int(n), pad, SENT[dtype]
        self.buf = torch.full((self.n + 2 * pad,), self.sent, dtype=dtype, device=dev)
        self.v = self.buf[pad:pad + self.n]

    @property
    def ptr(self):
        return self.v.data_ptr() if self.n else self.buf.data_ptr() + self.pad * self.buf.element_size()

    def np(self):
        return self.v.cpu().numpy()

    def check(self, label):
        assert bool((self.buf[:self.pad] == self.sent).all()) and bool((self.buf[self.pad + self.n:] == self.sent).all()), \
            f'{label}: a launch wrote outside its buffer'

    def untouched(self, label, start=0):
        assert bool((self.v[start:] == self.sent).all()), f'{label}: rows past the reported count were written'


def _in(dev, a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(dev)


def _sync():
    torch.cuda.synchronize()


def _cap_for(n):
    """the smallest legal capacity: the least power of two greater than n"""
    c = 1
    while c <= n:
        c *= 2
    return c


def _product_cap(n):
    """2n + 2 rounded up to a power of two (the load the product's host layer uses)"""
    return _cap_for(2 * n + 1)


def _rng(seed):
    return np.random.default_rng(seed)


def random_set(rng, n, n_batch, ts=1, span=12, empty=()):
    """unique, batch-major keys on multiples of ts (negative coordinates included); samples in `empty` have no rows"""
    live = [b for b in range(n_batch) if b not in empty]
    if not live or n == 0:
        return np.zeros(0, dtype=np.int64)
    b = np.sort(rng.choice(live, size=n))
    c = rng.integers(-span, span, size=(n, 3)) * ts
    keys, _ = S.unique_first(S.pack(b, c[:, 0], c[:, 1], c[:, 2]))
    return keys[np.argsort(keys >> 54, kind='stable')]


# ------------------------------------------------------------------------------------------------------------------ launch helpers
def run_unique_first(dev, keys, cap, with_src=True, label='unique_first'):
    """-> (count, out_keys Buf, out_src Buf, tkeys, tvals) checked against the specification"""
    hip = _hip()
    n = len(keys)
    kd = _in(dev, keys) if n else torch.zeros(1, dtype=torch.int64, device=dev)
    tk, tv = Buf(dev, cap, torch.int64), Buf(dev, cap)
    scratch = Buf(dev, 2 * n + n // 2048 + 4)
    ok, osrc = Buf(dev, n, torch.int64), Buf(dev, n)
    cnt = ctypes.c_int(-5)
    hip.call('es_unique_first', kd.data_ptr(), n, tk.ptr, tv.ptr, cap, scratch.ptr, ok.ptr, osrc.ptr if with_src else 0, ctypes.addressof(cnt), _st())
    _sync()
    for b in (tk, tv, scratch, ok, osrc):
        b.check(label)
    wk, ws = S.unique_first(keys)
    assert cnt.value == len(wk), f'{label}: count {cnt.value}, specified {len(wk)}'
    S.same(f'{label} out_keys', ok.np()[:len(wk)], wk)
    ok.untouched(label, len(wk))
    if with_src:
        S.same(f'{label} out_src', osrc.np()[:len(wk)], ws)
        osrc.untouched(label, len(wk))
    else:
        osrc.untouched(f'{label} (out_src = NULL)')
    S.check_table(label, tk.np(), tv.np(), wk, FILL_UNIQUE)
    return wk, tk, tv


def run_build_table(dev, keys, cap, label='build_table'):
    hip = _hip()
    n = len(keys)
    kd = _in(dev, keys) if n else torch.zeros(1, dtype=torch.int64, device=dev)
    tk, tv = Buf(dev, cap, torch.int64), Buf(dev, cap)
    hip.call('es_build_table', kd.data_ptr(), n, tk.ptr, tv.ptr, cap, _st())
    _sync()
    tk.check(label), tv.check(label)
    S.check_table(label, tk.np(), tv.np(), keys, FILL_BUILD)
    return tk, tv


def run_kernel_map(dev, out_keys, in_keys, tk, tv, cap, ksize, in_ts, label='kernel_map'):
    """-> nbr (n_out, K), checked against the specification"""
    hip = _hip()
    n_out, K = len(out_keys), ksize ** 3
    od = _in(dev, out_keys) if n_out else torch.zeros(1, dtype=torch.int64, device=dev)
    nbr = Buf(dev, n_out * K)
    hip.call('es_kernel_map', od.data_ptr(), n_out, tk.ptr, tv.ptr, cap, ksize, in_ts, nbr.ptr, _st())
    _sync()
    nbr.check(label)
    got = nbr.np().reshape(n_out, K)
    S.same(label, got, S.kernel_map(out_keys, in_keys, ksize, in_ts).reshape(n_out, K))
    return got, nbr


def run_inverse_map(dev, nbr_buf, nbr, n_in, label='inverse_map'):
    hip = _hip()
    n_out, K = nbr.shape
    inv = Buf(dev, n_in * K)
    hip.call('es_inverse_map', nbr_buf.ptr, n_out, K, n_in, inv.ptr, _st())
    _sync()
    inv.check(label)
    got = inv.np().reshape(n_in, K)
    S.same(label, got, S.inverse_map(nbr, n_in))
    return got


def absent_keys(rng, present, n):
    """n in-field keys that are not in `present`"""
    have = set(np.asarray(present).tolist())
    c = rng.integers(S.LO, S.HI + 1, size=(2 * n + 8, 3))
    q = S.pack(rng.integers(0, S.MAX_BATCH, size=len(c)), c[:, 0], c[:, 1], c[:, 2])
    q = np.array([k for k in q.tolist() if k not in have][:n], dtype=np.int64)
    assert len(q) == n
    return q


def lookups(dev, rng, unique_keys, tk, tv, cap, label):
    """every present key and as many absent ones through the device's own probe (es_kernel_map, one tap)"""
    q = np.concatenate([unique_keys, absent_keys(rng, unique_keys, max(len(unique_keys), 8))])
    q = q[rng.permutation(len(q))]
    got, _ = run_kernel_map(dev, q, unique_keys, tk, tv, cap, 1, 1, f'{label} lookups')
    assert int((got >= 0).sum()) == len(unique_keys)


# ------------------------------------------------------------------------------------------------------------------ hash table
MIX1, MIX2, M64 = 0xbf58476d1ce4e5b9, 0x94d049bb133111eb, (1 << 64) - 1


def splitmix64(keys):
    """numpy restatement of the table's hash (the splitmix64 finaliser), before masking"""
    x = np.asarray(keys, dtype=np.int64).view(np.uint64).copy()
    x ^= x >> np.uint64(30)
    x *= np.uint64(MIX1)
    x ^= x >> np.uint64(27)
    x *= np.uint64(MIX2)
    x ^= x >> np.uint64(31)
    return x


def _unxorshift(v, s):
    r = v
    for _ in range(64 // s + 1):
        r = v ^ (r >> s)
    return r


def keys_hashing_to_last_slot(rng, n, cap):
    """n distinct non-negative keys whose hash lands on slot cap - 1: the finaliser is a bijection, so it is run backwards from random
    images with the low bits set (Python integers), and the numpy restatement confirms every key"""
    out, seen = [], set()
    inv1, inv2 = pow(MIX1, -1, 1 << 64), pow(MIX2, -1, 1 << 64)
    while len(out) < n:
        h = (int(rng.integers(0, 1 << 62)) << 2 | int(rng.integers(0, 4))) | (cap - 1)
        x = _unxorshift(h, 31) * inv2 & M64
        x = _unxorshift(x, 27) * inv1 & M64
        x = _unxorshift(x, 30)
        if x < (1 << 63) and x not in seen:
            seen.add(x)
            out.append(x)
    keys = np.array(out, dtype=np.int64)
    assert np.all((splitmix64(keys) & np.uint64(cap - 1)) == np.uint64(cap - 1))
    return keys


def distinct_keys(rng, n):
    c = rng.integers(S.LO, S.HI + 1, size=(n + n // 8 + 8, 3))
    k, _ = S.unique_first(S.pack(rng.integers(0, S.MAX_BATCH, size=len(c)), c[:, 0], c[:, 1], c[:, 2]))
    assert len(k) >= n
    return k[:n]


TABLE_LOADS = [(1, 'product'), (1, 'least'), (300, 'product'), (1023, 'least'), (1024, 'least'), (4095, 'least')]


def table_case(dev, n, load, kind, seed, with_src):
    rng = _rng(seed)
    cap = _cap_for(n) if load == 'least' else _product_cap(n)
    label = f'table n={n} cap={cap} {kind}'
    if kind == 'wrap':
        keys = keys_hashing_to_last_slot(rng, n, cap)
    elif kind == 'equal':
        keys = np.full(n, int(distinct_keys(rng, 1)[0]), dtype=np.int64)
    elif kind == 'distinct':
        keys = distinct_keys(rng, n)
    else:                                                        # duplicates: about three occurrences of each key, shuffled
        base = distinct_keys(rng, max(n // 3, 1))
        keys = base[rng.integers(0, len(base), size=n)]
    uk, tk, tv = run_unique_first(dev, keys, cap, with_src=with_src, label=label)
    lookups(dev, rng, uk, tk, tv, cap, label)
    if kind != 'equal':
        tk2, tv2 = run_build_table(dev, uk, cap, label=label + ' build')
        lookups(dev, rng, uk, tk2, tv2, cap, label + ' build')


@pytest.mark.parametrize('kind', ['wrap', 'equal', 'distinct', 'dups'])
def test_hash_table_at_every_load(dev, kind):
    """cap = 2n + 2 as the product uses and the smallest legal cap, n = 1 .. 4095: adversarial keys that all hash to the last slot (the
    probe wraps), n equal keys (atomicMin contention), all distinct, duplicates; out_src NULL in every other case; lookups of every present key
    and as many absent ones on each table"""
    for i, (n, load) in enumerate(TABLE_LOADS):
        table_case(dev, n, load, kind, 10 * i + len(kind), with_src=(i + len(kind)) % 2 == 0)


def test_hash_table_refuses_a_bad_capacity(dev):
    """cap not a power of two, cap <= n, cap <= 0: -4 on the host, nothing written (fixed library only: the refusals return before any
    launch; without them a full table never lets an insert return)"""
    keys = distinct_keys(_rng(3), 64)
    kd = _in(dev, keys)
    tk, tv, scr, ok, osrc, nbr, fw = Buf(dev, 128, torch.int64), Buf(dev, 128), Buf(dev, 2 * 64 + 4), Buf(dev, 64, torch.int64), Buf(dev, 64), \
        Buf(dev, 64 * 8), Buf(dev, 64 * 8, torch.float32)
    cnt = ctypes.c_int(-5)
    off = _in(dev, np.array([0, 64], dtype=np.int32))
    st = _st()
    for cap in (0, -8, 96, 64, 32, 127):
        assert _rc('es_unique_first', kd.data_ptr(), 64, tk.ptr, tv.ptr, cap, scr.ptr, ok.ptr, osrc.ptr, ctypes.addressof(cnt), st) == -4
        assert _rc('es_build_table', kd.data_ptr(), 64, tk.ptr, tv.ptr, cap, st) == -4
        assert _rc('es_union_plan', kd.data_ptr(), 64, tk.ptr, tv.ptr, cap, kd.data_ptr(), 64, off.data_ptr(), off.data_ptr(), 1, scr.ptr, osrc.ptr,
                   osrc.ptr, ok.ptr, ctypes.addressof(cnt), st) == -4
        caps = (ctypes.c_int * 1)(cap)
        ptr1 = lambda b: (ctypes.c_void_p * 1)(b.ptr)
        res = (ctypes.c_int * 3)()
        assert _rc('es_strided_chain', kd.data_ptr(), 64, 1, 1, (ctypes.c_int * 1)(2), ok.ptr, scr.ptr, ptr1(tk), ptr1(tv), caps, ptr1(ok), osrc.ptr,
                   res, st) == -4
    for cap in (0, -8, 96, 127):
        assert _rc('es_kernel_map', kd.data_ptr(), 64, tk.ptr, tv.ptr, cap, 2, 1, nbr.ptr, st) == -4
        assert _rc('es_interp_map', kd.data_ptr(), 64, tk.ptr, tv.ptr, cap, 2, nbr.ptr, fw.ptr, st) == -4
    _sync()
    for b in (tk, tv, scr, ok, osrc, nbr, fw):
        b.check('refusal'), b.untouched('refusal')


# ------------------------------------------------------------------------------------------------------------------ scan
SCAN_NS = [1, 2047, 2048, 2049, 524288, 524289, 2 * 524288 + 3]
SCAN_FLAGS = ['zeros', 'ones', 'random']


def _flags(rng, n, kind):
    return {'zeros': np.zeros(n, dtype=np.int32), 'ones': np.ones(n, dtype=np.int32)}.get(kind, rng.integers(0, 2, size=n).astype(np.int32))


def _cheap_keys(rng, n):
    """n distinct in-field keys without a de-duplication pass (a random base plus a step along z and y)"""
    i = np.arange(n, dtype=np.int64)
    return S.pack(np.full(n, int(rng.integers(0, S.MAX_BATCH))), np.full(n, int(rng.integers(S.LO, S.HI))), S.LO + i // 4096, S.LO + i % 4096)


def compact_case(dev, n, kind, seed, count=True):
    hip = _hip()
    rng = _rng(seed)
    label = f'compact n={n} {kind}'
    keys, mask = _cheap_keys(rng, n), _flags(rng, n, kind)
    kd, md = _in(dev, keys), _in(dev, mask)
    scratch = Buf(dev, n + n // 2048 + 4)
    ok, osrc = Buf(dev, n, torch.int64), Buf(dev, n)
    cnt = ctypes.c_int(-5)
    hip.call('es_compact_mask', kd.data_ptr(), n, md.data_ptr(), scratch.ptr, ok.ptr, osrc.ptr, ctypes.addressof(cnt) if count else 0, _st())
    _sync()
    for b in (scratch, ok, osrc):
        b.check(label)
    wk, ws = S.compact_mask(keys, mask)
    assert not count or cnt.value == len(wk), f'{label}: count {cnt.value}, specified {len(wk)}'
    S.same(label + ' keys', ok.np()[:len(wk)], wk)
    S.same(label + ' src', osrc.np()[:len(wk)], ws)
    ok.untouched(label, len(wk)), osrc.untouched(label, len(wk))


@pytest.mark.parametrize('n', SCAN_NS)
def test_scan_through_compact_mask(dev, n):
    for i, kind in enumerate(SCAN_FLAGS):
        compact_case(dev, n, kind, n % 1000 + i, count=(i != 1 or n != 2049))


def scan_unique_keys(rng, n, kind):
    """winner flags all 1 (distinct keys), one 1 then 0s ('zeros': n equal keys -- the first occurrence is always flagged) or random"""
    if kind == 'ones':
        return _cheap_keys(rng, n)
    if kind == 'zeros':
        return np.full(n, int(_cheap_keys(rng, 1)[0]), dtype=np.int64)
    base = _cheap_keys(rng, max(n // 2, 1))
    return base[rng.integers(0, len(base), size=n)]


@pytest.mark.parametrize('n', SCAN_NS)
def test_scan_through_unique_first(dev, n):
    for i, kind in enumerate(SCAN_FLAGS):
        run_unique_first(dev, scan_unique_keys(_rng(n % 1000 + i), n, kind), _product_cap(n), label=f'unique_first n={n} {kind}')


def run_union(dev, ka, kb, n_batch, cap=None, label='union'):
    hip = _hip()
    na, nb = len(ka), len(kb)
    cap = cap or _product_cap(na)
    tk, tv = run_build_table(dev, ka, cap, label=label + ' table')
    kad = _in(dev, ka) if na else torch.zeros(1, dtype=torch.int64, device=dev)
    kbd = _in(dev, kb) if nb else torch.zeros(1, dtype=torch.int64, device=dev)
    aoff, boff = _in(dev, S.batch_offsets(ka, n_batch)), _in(dev, S.batch_offsets(kb, n_batch))
    scratch = Buf(dev, 3 * nb + nb // 2048 + 4)
    pa, pb, ok = Buf(dev, na), Buf(dev, nb), Buf(dev, na + nb, torch.int64)
    cnt = ctypes.c_int(-5)
    hip.call('es_union_plan', kad.data_ptr(), na, tk.ptr, tv.ptr, cap, kbd.data_ptr(), nb, aoff.data_ptr(), boff.data_ptr(), n_batch, scratch.ptr,
             pa.ptr, pb.ptr, ok.ptr, ctypes.addressof(cnt), _st())
    _sync()
    for b in (scratch, pa, pb, ok, tk, tv):
        b.check(label)
    wa, wb, wk, wn = S.union_plan(ka, kb, n_batch)
    assert cnt.value == wn, f'{label}: count {cnt.value}, specified {wn}'
    S.same(label + ' pos_a', pa.np(), wa)
    S.same(label + ' pos_b', pb.np(), wb)
    S.same(label + ' out_keys', ok.np()[:wn], wk)
    ok.untouched(label, wn)
    b_out = wk >> 54
    assert np.all(b_out[1:] >= b_out[:-1]), f'{label}: the specified union is not batch-major'


def grid_set(rng, n, n_batch, x0):
    """n distinct batch-major keys without a de-duplication pass: cell i of a 128 x 128 x ... block at x >= x0, random samples"""
    i = np.arange(n, dtype=np.int64)
    return S.pack(np.sort(rng.integers(0, n_batch, size=n)), x0 + i % 128, i // 128 % 128 - 64, i // 16384 - 32)


def union_sets(rng, nb, kind, n_batch=3):
    """a, b (|b| = nb exactly) with the new-row flags of b all 0 (b inside a), all 1 (disjoint) or random"""
    kb = grid_set(rng, nb, n_batch, -64)
    other = grid_set(rng, nb // 2 + 8, n_batch, 1000)                             # disjoint from b
    if kind == 'zeros':
        ka = np.concatenate([kb, other])
    elif kind == 'ones':
        ka = other
    else:
        ka = np.concatenate([kb[rng.random(nb) < 0.5], other])
    ka = ka[rng.permutation(len(ka))]
    return ka[np.argsort(ka >> 54, kind='stable')], kb


@pytest.mark.parametrize('nb', SCAN_NS)
def test_scan_through_union_plan(dev, nb):
    for i, kind in enumerate(SCAN_FLAGS):
        ka, kb = union_sets(_rng(nb % 1000 + i), nb, kind)
        run_union(dev, ka, kb, 3, label=f'union nb={nb} {kind}')


def test_union_plan_with_empty_nested_disjoint_and_one_sided_operands(dev):
    rng = _rng(21)
    a = random_set(rng, 500, 4)
    for nbv in (2047, 2049):
        ka, kb = union_sets(rng, nbv, 'random', n_batch=4)
        run_union(dev, ka, kb, 4, label=f'union nb={nbv}')
    empty = np.zeros(0, dtype=np.int64)
    run_union(dev, empty, a, 4, cap=1, label='union a empty, least cap')
    run_union(dev, empty, a, 4, label='union a empty')
    run_union(dev, a, empty, 4, label='union b empty')
    run_union(dev, empty, empty, 4, label='union both empty')
    run_union(dev, a, a[rng.random(len(a)) < 0.3], 4, label='union b inside a')
    far = S.pack(*[v + d for v, d in zip(S.unpack(a), (0, 1000, 0, 0))])
    run_union(dev, a, far, 4, label='union disjoint')
    # samples present on one side only: a has rows in samples {0, 2}, b in {1, 2, 3}
    a2, b2 = random_set(rng, 300, 4, empty=(1, 3)), random_set(rng, 300, 4, empty=(0,))
    run_union(dev, a2, b2, 4, cap=_cap_for(len(a2)), label='union one-sided samples')
    run_union(dev, b2, a2, 4, label='union one-sided samples, swapped')


# ------------------------------------------------------------------------------------------------------------------ offsets, chain
N_BATCHES = [1, 2, 63, 64, 65, 255, 256, 300, S.MAX_BATCH]


def sample_layout(n_batch):
    """samples with no rows: the first, the last and a middle run (where n_batch allows)"""
    if n_batch < 4:
        return ()
    return (0, n_batch - 1, n_batch // 2, n_batch // 2 + 1)


def run_batch_offsets(dev, keys, n_batch, label):
    hip = _hip()
    kd = _in(dev, keys) if len(keys) else torch.zeros(1, dtype=torch.int64, device=dev)
    off = Buf(dev, n_batch + 1)
    hip.call('es_batch_offsets', kd.data_ptr(), len(keys), n_batch, off.ptr, _st())
    _sync()
    off.check(label)
    S.same(label, off.np(), S.batch_offsets(keys, n_batch))


def run_chain(dev, root, n_batch, ts_list, label, least_cap=False):
    hip = _hip()
    n, L = len(root), len(ts_list)
    cap = _cap_for(n) if least_cap else _product_cap(n)
    rd = _in(dev, root) if n else torch.zeros(1, dtype=torch.int64, device=dev)
    tmp, scratch = Buf(dev, n, torch.int64), Buf(dev, 2 * n + n // 2048 + 8)
    tks, tvs, oks = [Buf(dev, cap, torch.int64) for _ in range(L)], [Buf(dev, cap) for _ in range(L)], [Buf(dev, n, torch.int64) for _ in range(L)]
    per = n_batch + 2
    res_dev = Buf(dev, L * per)
    res_host = (ctypes.c_int * (L * per + 2))(*([-5] * (L * per + 2)))
    ptrs = lambda bs: (ctypes.c_void_p * L)(*[b.ptr for b in bs])
    hip.call('es_strided_chain', rd.data_ptr(), n, n_batch, L, (ctypes.c_int * L)(*ts_list), tmp.ptr, scratch.ptr, ptrs(tks), ptrs(tvs),
             (ctypes.c_int * L)(*([cap] * L)), ptrs(oks), res_dev.ptr, res_host, _st())
    _sync()
    for b in [tmp, scratch, res_dev] + tks + tvs + oks:
        b.check(label)
    levels, res = S.strided_chain(root, n_batch, ts_list)
    got = np.array(res_host[:])
    assert np.all(got[L * per:] == -5), f'{label}: res_host written past n_levels * (n_batch + 2)'
    if n == 0:
        assert np.all(got[:L * per] == 0), f'{label}: n = 0 must report zero counts and offsets'
        return
    S.same(label + ' res_host', got[:L * per], res)
    S.same(label + ' res_dev', res_dev.np(), res)
    for l in range(L):
        S.same(f'{label} level {l} keys', oks[l].np()[:len(levels[l])], levels[l])
        oks[l].untouched(f'{label} level {l}', len(levels[l]))
        S.check_table(f'{label} level {l}', tks[l].np(), tvs[l].np(), levels[l], FILL_UNIQUE)


@pytest.mark.parametrize('n_batch', N_BATCHES)
def test_batch_offsets_chain_and_union_over_sample_counts(dev, n_batch):
    """one workgroup serves every offset: n_batch + 1 above its 64 / 256 threads needs the loop over b"""
    rng = _rng(n_batch)
    empty = sample_layout(n_batch)
    keys = random_set(rng, 3 * n_batch + 40, n_batch, empty=empty)
    label = f'n_batch={n_batch}'
    run_batch_offsets(dev, keys, n_batch, label + ' offsets')
    run_batch_offsets(dev, keys[:0], n_batch, label + ' offsets n=0')
    run_chain(dev, keys, n_batch, [2], label + ' chain L=1')
    if n_batch in (2, 65, 300, S.MAX_BATCH):
        run_chain(dev, keys, n_batch, [2, 4, 8, 16, 32, 64], label + ' chain L=6', least_cap=True)
        run_chain(dev, keys[:0], n_batch, [2, 4], label + ' chain n=0')
    other = random_set(rng, 2 * n_batch + 40, n_batch, empty=empty[:1] + tuple(range(1, n_batch, 7)))
    run_union(dev, keys, other, n_batch, label=label + ' union')


def test_sample_counts_above_the_maximum_are_refused(dev):
    keys = random_set(_rng(5), 100, 4)
    kd = _in(dev, keys)
    nbad = S.MAX_BATCH + 1
    off, scr, ok, tk, tv = Buf(dev, nbad + 1), Buf(dev, 3 * 100 + 8), Buf(dev, 200, torch.int64), Buf(dev, 256, torch.int64), Buf(dev, 256)
    cnt = ctypes.c_int(-5)
    st = _st()
    assert _hip().CONSTS['ES_MAX_BATCH'] == S.MAX_BATCH
    assert _rc('es_batch_offsets', kd.data_ptr(), 100, nbad, off.ptr, st) == -4
    ptr1 = lambda b: (ctypes.c_void_p * 1)(b.ptr)
    res = (ctypes.c_int * (nbad + 2))()
    assert _rc('es_strided_chain', kd.data_ptr(), 100, nbad, 1, (ctypes.c_int * 1)(2), ok.ptr, scr.ptr, ptr1(tk), ptr1(tv), (ctypes.c_int * 1)(256),
               ptr1(ok), off.ptr, res, st) == -4
    assert _rc('es_union_plan', kd.data_ptr(), 100, tk.ptr, tv.ptr, 256, kd.data_ptr(), 100, off.ptr, off.ptr, nbad, scr.ptr, scr.ptr, scr.ptr, ok.ptr,
               ctypes.addressof(cnt), st) == -4
    pts = torch.zeros(4, 3, device=dev)
    assert _rc('es_voxel_keys', pts.data_ptr(), 4, 3, S.MAX_BATCH, 0.01, ok.ptr, st) == -4
    assert _rc('es_voxel_keys', pts.data_ptr(), 4, 3, -1, 0.01, ok.ptr, st) == -4
    assert _rc('es_voxel_keys_range', pts.data_ptr(), 4, 3, S.MAX_BATCH, (ctypes.c_float * 9)(*([1.0] * 9)), ok.ptr, st) == -4
    _sync()
    for b in (off, scr, ok, tk, tv):
        b.check('refusal'), b.untouched('refusal')


# ------------------------------------------------------------------------------------------------------------------ kernel maps
def map_case(dev, rng, ksize, in_ts, same_set, via_unique, n_in=331, n_out=37, label=''):
    ins = random_set(rng, n_in, 3, ts=in_ts, span=5)
    if same_set:
        outs = ins
    else:
        outs = random_set(rng, n_out, 3, ts=in_ts * 2, span=3)
        outs, _ = S.unique_first(np.concatenate([outs, S.stride_keys(ins[:n_out], in_ts * 2)]))
        outs = outs[np.argsort(outs >> 54, kind='stable')][:n_out]
    cap = _cap_for(len(ins)) if via_unique else _product_cap(len(ins))
    if via_unique:
        _, tk, tv = run_unique_first(dev, ins, cap, label=label + ' table')
    else:
        tk, tv = run_build_table(dev, ins, cap, label=label + ' table')
    nbr, nbuf = run_kernel_map(dev, outs, ins, tk, tv, cap, ksize, in_ts, label + ' nbr')
    inv = run_inverse_map(dev, nbuf, nbr, len(ins), label + ' inv')
    assert int((nbr >= 0).sum()) > 0
    if same_set and ksize % 2:
        K = ksize ** 3
        S.same(label + ' mirror identity', inv, nbr[:, ::-1])
        S.same(label + ' centre tap', nbr[:, K // 2], np.arange(len(ins), dtype=np.int32))
    return nbr


@pytest.mark.parametrize('in_ts', [1, 2, 8, 64])
def test_kernel_and_inverse_maps_on_the_kernel_and_stride_grid(dev, in_ts):
    rng = _rng(in_ts)
    sizes = 0
    for ksize in (1, 2, 3):
        for same_set in (True, False):
            for via_unique in (False, True):
                nbr = map_case(dev, rng, ksize, in_ts, same_set, via_unique, label=f'map k={ksize} ts={in_ts} same={same_set} unique={via_unique}')
                sizes += nbr.size % 256 != 0
    assert sizes > 0, 'no map whose n_out K is not a multiple of the workgroup size'


def test_kernel_and_inverse_maps_with_empty_operands(dev):
    rng = _rng(77)
    ins = random_set(rng, 100, 2)
    empty = np.zeros(0, dtype=np.int64)
    tk, tv = run_build_table(dev, ins, 128, label='empty-operand table')
    nbr, nbuf = run_kernel_map(dev, empty, ins, tk, tv, 128, 3, 1, 'n_out = 0')
    run_inverse_map(dev, nbuf, nbr, len(ins), 'inverse of n_out = 0')            # all -1: the memset alone
    tk0, tv0 = run_build_table(dev, empty, 1, label='table of nothing, cap 1')
    nbr, nbuf = run_kernel_map(dev, ins, empty, tk0, tv0, 1, 3, 1, 'n_in = 0')
    assert np.all(nbr == -1)
    run_inverse_map(dev, nbuf, nbr, 0, 'inverse with n_in = 0')


def edge_keys():
    """the field's corners: for each axis a voxel at LO and one at HI in sample 0, plus the voxel of sample 1 / the next x / the next y
    row that a carry out of that axis' field would reach"""
    L, H = S.LO, S.HI
    return S.pack([0, 0, 1, 0, 0, 0, 0, 0],
                  [0, H, L, 0, 1, 5, 0, 5],
                  [0, 0, 0, H, L, 5, 0, 6],
                  [L, 0, 0, 0, 0, H, 0, L])


@pytest.mark.parametrize('via_unique', [False, True])
def test_three_key_edge_of_the_field(dev, via_unique):
    """(0; 0,0,LO), (0; HI,0,0), (1; LO,0,0) and the y / z analogues under a 3^3 map at stride 1: a +1 step off HI packs into the next
    field (x: the next SAMPLE), a -1 step off z = LO packs to the empty key -1, which matched an empty slot and returned its fill"""
    keys = edge_keys()
    assert len(set(keys.tolist())) == len(keys)
    order = np.argsort(keys >> 54, kind='stable')
    keys = keys[order]
    cap = 16
    if via_unique:
        _, tk, tv = run_unique_first(dev, keys, cap, label='edge table')
    else:
        tk, tv = run_build_table(dev, keys, cap, label='edge table')
    for ksize in (3, 2):
        nbr, _ = run_kernel_map(dev, keys, keys, tk, tv, cap, ksize, 1, f'edge map k={ksize} unique={via_unique}')
        if ksize == 3:
            S.same('edge map: every voxel is alone', nbr, np.where(np.arange(27)[None] == 13, np.arange(len(keys))[:, None], -1).astype(np.int32))


# ------------------------------------------------------------------------------------------------------------------ stride / interp / children
def edge_coordinate_values(ts):
    return np.array([-ts - 1, -ts, -ts + 1, -1, 0, 1, ts - 1, ts, ts + 1, S.LO, S.HI], dtype=np.int64)


@pytest.mark.parametrize('ts', [2, 4, 8, 16, 32, 64])
def test_stride_keys_and_interp_map_at_every_stride(dev, ts):
    hip = _hip()
    rng = _rng(ts)
    v = edge_coordinate_values(ts)
    x, y, z = (g.reshape(-1) for g in np.meshgrid(v, v, v, indexing='ij'))
    q = S.pack(rng.integers(0, 2, size=len(x)) * (S.MAX_BATCH - 1), x, y, z)
    n = len(q)
    qd = _in(dev, q)
    out = Buf(dev, n, torch.int64)
    hip.call('es_stride_keys', qd.data_ptr(), n, ts, out.ptr, _st())
    _sync()
    out.check('stride_keys')
    floored = S.stride_keys(q, ts)
    S.same(f'stride_keys ts={ts}', out.np(), floored)
    # the table: the cells' corners, a third of them dropped (absent corners), plus the highest in-field corner row
    corners, _ = S.unique_first(np.concatenate([floored, S.gen_children(floored, ts)]))
    corners = corners[(corners != S.ABSENT_KEY) & (rng.random(len(corners)) < 0.67)]
    cap = _cap_for(len(corners))
    tk, tv = run_build_table(dev, corners, cap, label=f'interp table ts={ts}')
    idx, w = Buf(dev, n * 8), Buf(dev, n * 8, torch.float32)
    hip.call('es_interp_map', qd.data_ptr(), n, tk.ptr, tv.ptr, cap, ts, idx.ptr, w.ptr, _st())
    _sync()
    idx.check('interp idx'), w.check('interp w')
    widx, ww = S.interp_map(q, corners, ts)
    S.same(f'interp_map ts={ts} idx', idx.np().reshape(n, 8), widx)
    S.same(f'interp_map ts={ts} weights', w.np().reshape(n, 8), ww)
    top = (x + ts > S.HI) | (y + ts > S.HI) | (z + ts > S.HI)                     # queries in the last cell: their upper corners do not exist
    assert top.any() and np.all(widx[x == S.HI][:, 1::2] == -1) and int((widx >= 0).sum()) > n


def test_gen_children_keys_inside_and_at_the_end_of_the_field(dev):
    hip = _hip()
    rng = _rng(8)
    for half in (1, 4, 32):
        ts = 2 * half
        inner = random_set(rng, 200, 3, ts=ts, span=6)
        last = S.HI + 1 - ts                                                    # the last multiple of ts: its children are in the field
        v = np.array([S.LO, last, S.HI - half + 1, S.HI, 0], dtype=np.int64)    # HI - half + 1, HI: unaligned parents whose +half child is not
        x, y, z = (g.reshape(-1) for g in np.meshgrid(v, v, v, indexing='ij'))
        keys = np.concatenate([inner, S.pack(np.full(len(x), S.MAX_BATCH - 1), x, y, z)])
        n = len(keys)
        out = Buf(dev, 8 * n, torch.int64)
        hip.call('es_gen_children_keys', _in(dev, keys).data_ptr(), n, half, out.ptr, _st())
        _sync()
        out.check('gen_children')
        want = S.gen_children(keys, half)
        S.same(f'gen_children half={half}', out.np(), want)
        assert np.all(want[:8 * len(inner)] >= 0) and int((want == S.ABSENT_KEY).sum()) > 0
        live = want[want >= 0]
        assert np.all((live >> 54) == np.repeat(keys >> 54, 8)[want >= 0]), 'a child left its sample'


def test_keys_to_coords_and_points(dev):
    hip = _hip()
    rng = _rng(9)
    for n, vs in ((1, 0.01), (257, 0.02), (1000, 0.16)):
        c = rng.integers(S.LO, S.HI + 1, size=(n, 3))
        c[:min(n, 2)] = [[S.LO, S.HI, 0], [S.HI, S.LO, -1]][:min(n, 2)]
        keys = S.pack(rng.integers(0, S.MAX_BATCH, size=n), c[:, 0], c[:, 1], c[:, 2])
        coords, pts = Buf(dev, 4 * n), Buf(dev, 3 * n, torch.float32)
        hip.call('es_keys_to_coords', _in(dev, keys).data_ptr(), n, coords.ptr, _st())
        hip.call('es_coords_to_points', coords.ptr, n, vs, pts.ptr, _st())
        _sync()
        coords.check('keys_to_coords'), pts.check('coords_to_points')
        want = S.keys_to_coords(keys)
        S.same('keys_to_coords', coords.np().reshape(n, 4), want)
        S.same('coords_to_points', pts.np().reshape(n, 3), S.coords_to_points(want, vs))
        S.same('pack(unpack)', S.pack(*S.unpack(keys)), keys)


# ------------------------------------------------------------------------------------------------------------------ sort
SORT_NS = [1, 2, 255, 256, 257, 2047, 2048, 2049, 32768, 32769, 262144 + 300]


def sort_keys(rng, n, pattern):
    """'bit62' / 'full64': the top bits, up to the sign bit (the sort orders unsigned 64-bit values).  'bit61': 62 random bits with bit 61 set (8 non-trivial passes: even); 'equal'; ('digit', p): keys that differ in
    digit p only (1 pass: odd -- the result lies in the other buffer); ('digits', p, q): two non-trivial passes; 'dups': 7 distinct keys"""
    if pattern == 'bit61':
        return (rng.integers(0, 1 << 61, size=n) | (1 << 61)).astype(np.int64)
    if pattern == 'bit62':                                                      # past the 2^62 the header used to name
        return (rng.integers(0, 1 << 62, size=n) | (1 << 62)).astype(np.int64)
    if pattern == 'full64':                                                     # every bit random, the sign bit included: unsigned order
        return rng.integers(0, 1 << 64, size=n, dtype=np.uint64).view(np.int64)
    base = int(rng.integers(0, 1 << 61)) | (1 << 61)
    if pattern == 'equal':
        return np.full(n, base, dtype=np.int64)
    if pattern == 'dups':
        return rng.integers(0, 7, size=n).astype(np.int64) * 1000003
    keys = np.full(n, base, dtype=np.uint64)
    for p in pattern[1:]:                                                       # (digit 7 reaches bits 62 and 63: unsigned order)
        keys = (keys & ~np.uint64(255 << (8 * p))) | (rng.integers(0, 256, size=n).astype(np.uint64) << np.uint64(8 * p))
    keys = keys.view(np.int64)
    return keys


def run_sort(dev, name, keys, src, label, short=0):
    """es_sort_u64 / es_morton_sort with scratch of exactly es_sort_scratch_bytes(n) (src None: NULL)"""
    hip = _hip()
    n = len(keys)
    nbytes = int(hip.raw('es_sort_scratch_bytes')(n))
    scratch = Buf(dev, nbytes, torch.uint8, pad=256)
    ok, osrc = Buf(dev, n, torch.int64), Buf(dev, n)
    kd = _in(dev, keys)
    sd = _in(dev, src) if src is not None else None
    rc = _rc(name, kd.data_ptr(), sd.data_ptr() if sd is not None else 0, n, scratch.ptr, nbytes - short, ok.ptr, osrc.ptr, _st())
    _sync()
    for b in (scratch, ok, osrc):
        b.check(label)
    if short:
        assert rc == -5, f'{label}: scratch one byte short returned {rc}'
        ok.untouched(label), osrc.untouched(label), scratch.untouched(label)
        return
    assert rc == 0, f'{label}: status {rc}'
    wk, ws = (S.sort_u64 if name == 'es_sort_u64' else S.morton_sort)(keys, src)
    S.same(label + ' keys', ok.np(), wk)
    if src is not None:
        S.same(label + ' src', osrc.np(), ws)
    else:
        osrc.untouched(label + ' (src = NULL)')


@pytest.mark.parametrize('n', SORT_NS)
def test_sort_u64_on_the_size_grid(dev, n):
    """full-width keys (every pass permutes) and 7 distinct keys under a REVERSED payload (stability) at every size where the tile count,
    the digit table (17 tiles x 256 digits pass the 4096-entry slab of its scan) or the histogram's workgroup stride changes"""
    rng = _rng(n % 997)
    rev = np.arange(n, dtype=np.int32)[::-1].copy()
    run_sort(dev, 'es_sort_u64', sort_keys(rng, n, 'bit61'), rng.permutation(n).astype(np.int32), f'sort n={n} bit61')
    run_sort(dev, 'es_sort_u64', sort_keys(rng, n, 'dups'), rev, f'sort n={n} dups')


@pytest.mark.parametrize('n', [257, 2049, 32769])
def test_sort_u64_pass_patterns_and_both_result_parities(dev, n):
    rng = _rng(n)
    rev = np.arange(n, dtype=np.int32)[::-1].copy()
    run_sort(dev, 'es_sort_u64', sort_keys(rng, n, 'equal'), rev, f'sort n={n} equal')
    for p in range(8):
        run_sort(dev, 'es_sort_u64', sort_keys(rng, n, ('digit', p)), rev, f'sort n={n} digit {p}')
    for p, q in ((0, 7), (3, 4)):
        run_sort(dev, 'es_sort_u64', sort_keys(rng, n, ('digits', p, q)), rev, f'sort n={n} digits {p},{q}')
    run_sort(dev, 'es_sort_u64', sort_keys(rng, n, ('digits', 1, 2, 5)), None, f'sort n={n} three digits, src NULL')
    run_sort(dev, 'es_sort_u64', sort_keys(rng, n, 'bit62'), rev, f'sort n={n} bit 62 set')
    run_sort(dev, 'es_sort_u64', sort_keys(rng, n, 'full64'), rev, f'sort n={n} all 64 bits')
    run_sort(dev, 'es_sort_u64', sort_keys(rng, n, 'bit61'), rev, f'sort n={n} short scratch', short=1)


def morton_inputs(rng, n):
    """unique keys of samples 0, 255 and 511, coordinates over the whole field with both ends of every axis present"""
    c = rng.integers(S.LO, S.HI + 1, size=(n + 16, 3))
    ends = np.array([[S.LO, S.LO, S.LO], [S.HI, S.HI, S.HI], [S.LO, S.HI, 0], [0, S.LO, S.HI], [S.HI, 0, S.LO], [-1, 0, -1], [0, -1, 0]])
    c[:len(ends)] = ends
    b = rng.choice([0, 255, S.MAX_BATCH - 1], size=len(c))
    b[:3] = [0, 255, S.MAX_BATCH - 1]
    keys, _ = S.unique_first(S.pack(b, c[:, 0], c[:, 1], c[:, 2]))
    return keys[:n]


@pytest.mark.parametrize('n', [1, 2, 257, 2049, 32769])
def test_morton_sort_over_the_whole_field_and_sample_range(dev, n):
    rng = _rng(n + 1)
    keys = morton_inputs(rng, n)
    run_sort(dev, 'es_morton_sort', keys, rng.permutation(len(keys)).astype(np.int32), f'morton n={n}')
    if n == 257:
        run_sort(dev, 'es_morton_sort', keys, None, 'morton src NULL')
        run_sort(dev, 'es_morton_sort', keys, None, 'morton short scratch', short=1)
        small = S.pack(rng.integers(0, 2, size=300), *(rng.integers(-2, 2, size=(3, 300))))       # duplicates: ties in input order
        run_sort(dev, 'es_morton_sort', small, np.arange(300, dtype=np.int32)[::-1].copy(), 'morton duplicates')


# ------------------------------------------------------------------------------------------------------------------ voxel keys
def _ulp_neighbours(v):
    v = np.asarray(v, dtype=np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(-np.inf)), np.nextafter(v, np.float32(np.inf))])


def voxel_points(vs, window=40):
    """every k vs for |k| <= window, the field's ends and one past them, each with its two f32 neighbours; huge values, +-inf, NaN"""
    f = np.float32
    k = np.concatenate([np.arange(-window, window + 1), [S.HI - 1, S.HI, S.HI + 1, S.LO + 1, S.LO, S.LO - 1]]).astype(np.float32)
    v = _ulp_neighbours(k * f(vs))
    wild = np.array([1e30, -1e30, 3.4e38, -3.4e38, np.inf, -np.inf, np.nan, 2.2e9 * vs, -2.2e9 * vs, 4.3e9 * vs, 1e-45, -1e-45, 0.0, -0.0], dtype=np.float32)
    return np.concatenate([v, wild])


@pytest.mark.parametrize('vs', [0.01, 0.02, 0.16])
def test_voxel_keys_around_every_boundary_and_outside_the_domain(dev, vs):
    hip = _hip()
    rng = _rng(int(vs * 100))
    v = voxel_points(vs)
    for ld in (3, 6):
        for batch in (0, S.MAX_BATCH - 1):
            pts = np.full((len(v), ld), np.float32(-777.25), dtype=np.float32)
            pts[:, 0], pts[:, 1], pts[:, 2] = v, v[rng.permutation(len(v))], v[rng.permutation(len(v))]
            keys = Buf(dev, len(v), torch.int64)
            hip.call('es_voxel_keys', _in(dev, pts).data_ptr(), len(v), ld, batch, vs, keys.ptr, _st())
            _sync()
            keys.check('voxel_keys')
            got = keys.np()
            S.same(f'voxel_keys vs={vs} ld={ld} batch={batch}', got, S.voxel_keys(pts, batch, vs))
            b, x, y, z = S.unpack(got)
            assert np.all(b == batch) and np.all(S.in_field(x, y, z)) and np.all(got >= 0)
    inside = np.abs(v) < 1000.0                                                  # in-domain finite points: plain truncation, as before
    with np.errstate(all='ignore'):
        plain = np.trunc(v[inside] / np.float32(vs)).astype(np.int64)
    S.same('in-domain rule', S.unpack(S.voxel_keys(np.stack([v[inside]] * 3, 1), 0, vs))[1], plain)


def test_voxel_keys_range_on_and_past_each_clamp_bound(dev):
    hip = _hip()
    rng = _rng(31)
    f = np.float32
    for ld, rngv in ((3, [-3.2, -3.2, -1.28, 0.16, 0.16, 0.16, 39, 39, 15]), (6, [-1.0, 0.5, 0.0, 0.01, 0.02, 0.16, 0, 1e9, 131071]),
                     (6, [0.0, 0.0, 0.0, 0.02, 0.02, 0.02, 7, float('inf'), -3])):
        r = np.array(rngv, dtype=np.float32)
        cols = []
        for a in range(3):
            k = np.concatenate([np.arange(-3, 4), [r[6 + a] - 1, r[6 + a], r[6 + a] + 1] if np.isfinite(r[6 + a]) and abs(r[6 + a]) < 1e6 else []]).astype(f)
            on = _ulp_neighbours(k * r[3 + a] + r[a])                            # on / just below / just above each cell and clamp bound
            frac = np.array([-0.9, -0.5, -1e-3], dtype=f) * r[3 + a] + r[a]      # quotients in (-1, 0): truncate to 0, not to -1
            wild = np.array([1e30, -1e30, np.inf, -np.inf, np.nan, 3e9 * r[3 + a], -3e9 * r[3 + a], 140000 * r[3 + a]], dtype=f)
            cols.append(np.concatenate([on, frac, wild]).astype(f))
        m = max(len(c) for c in cols)
        pts = np.full((m, ld), f(0.25), dtype=np.float32)
        for a in range(3):
            pts[:, a] = np.resize(cols[a], m)[rng.permutation(m)] if a else np.resize(cols[a], m)
        for batch in (0, S.MAX_BATCH - 1):
            keys = Buf(dev, m, torch.int64)
            hip.call('es_voxel_keys_range', _in(dev, pts).data_ptr(), m, ld, batch, (ctypes.c_float * 9)(*[float(t) for t in r]), keys.ptr, _st())
            _sync()
            keys.check('voxel_keys_range')
            got = keys.np()
            S.same(f'voxel_keys_range {rngv} batch={batch}', got, S.voxel_keys_range(pts, batch, r))
            b, x, y, z = S.unpack(got)
            assert np.all(b == batch) and np.all(S.in_field(x, y, z)) and np.all(np.stack([x, y, z]) >= 0)


# ------------------------------------------------------------------------------------------------------------------ dense
def test_dense_maps(dev):
    hip = _hip()
    seen_stride = 0
    for B, X, Y, Z in ((2, 5, 7, 3), (1, 27, 27, 27)):
        for ks, stride, pad in ((3, 1, 1), (3, 2, 1), (1, 2, 0), (1, 1, 0)):
            if X == 27 and (ks, stride) != (3, 1):
                continue
            Xo, Yo, Zo = ((v + 2 * pad - ks) // stride + 1 for v in (X, Y, Z))
            tot = B * Xo * Yo * Zo * ks ** 3
            seen_stride += tot > 2048 * 256
            nbr = Buf(dev, tot)
            hip.call('es_volume_map', B, X, Y, Z, Xo, Yo, Zo, ks, stride, pad, nbr.ptr, _st())
            _sync()
            nbr.check('volume_map')
            S.same(f'volume_map {(B, X, Y, Z)} {(ks, stride, pad)}', nbr.np().reshape(-1, ks ** 3), S.volume_map(B, X, Y, Z, Xo, Yo, Zo, ks, stride, pad))
    assert seen_stride == 1, 'no volume map past one sweep of its grid-stride loop'
    for B, X, Y, Z in ((2, 3, 5, 7), (1, 33, 32, 32)):
        tot = B * X * Y * Z * 8
        idx = Buf(dev, tot)
        hip.call('es_volume_up_index', B, X, Y, Z, idx.ptr, _st())
        _sync()
        idx.check('volume_up_index')
        S.same(f'volume_up_index {(B, X, Y, Z)}', idx.np(), S.volume_up_index(B, X, Y, Z))
    assert tot > 1024 * 256
    rng = _rng(41)
    X, Y, Z = 5, 7, 3
    for ts in (1, 8):
        vals = [np.array([-ts, -1, 0, ts - 1, ts, (d - 1) * ts, d * ts - 1, d * ts, d * ts + 1, (d + 1) * ts]) for d in (X, Y, Z)]
        x, y, z = (g.reshape(-1) for g in np.meshgrid(*vals, indexing='ij'))
        coords = np.stack([rng.integers(0, 3, size=len(x)), x, y, z], 1).astype(np.int32)
        n = len(coords)
        idx = Buf(dev, n)
        hip.call('es_dense_index', _in(dev, coords).data_ptr(), n, ts, X, Y, Z, idx.ptr, _st())
        _sync()
        idx.check('dense_index')
        want = S.dense_index(coords, ts, X, Y, Z)
        S.same(f'dense_index ts={ts}', idx.np(), want)
        assert int((want >= 0).sum()) > 0 and int((want < 0).sum()) > 0
