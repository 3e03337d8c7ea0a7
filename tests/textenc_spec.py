"""Specifications of the frozen text encoder's kernels (csrc/transformer.hip: es_text_attn_fwd, es_text_embed_ln, es_bias_gelu), evaluated
in f64 in the style of tests/fwd_spec.py: u = 2^-24, G = 8, per-element bounds, none of which depends on 1 / |spec|; a Stats object
collects the worst ratio.  The *_ref functions are plain f32 evaluations of the formulas (with optional mutations: a correct output with
one thing wrong) -- tests/test_emu_textenc.py asserts that every checker accepts the former and rejects the latter."""
import math

import torch

from fwd_spec import F64, G, U, Stats, _d, _fail_at, _r  # noqa: F401  (Stats is re-exported for the tests)

D = 64
SCALE = 0.125                       # 1 / sqrt(64): a power of two, so scaling commutes with the bf16 rounding


def _held(label, got, want, bound, cls, stats):
    """assert |got - want| <= bound element by element; the class's worst ratio is G max(|err| / bound): the bound is used up at G = 8"""
    got = got.to(F64)
    err = (got - want).abs()
    if bool((~(err <= bound)).any()):
        _fail_at(label, err, bound, got, want)
    pos = bound > 0
    ratio = G * float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    stats.note(cls, ratio, float((got - want).norm() / (want.norm() + 1e-300)))
    return ratio


def _heads(t, B, T, H):
    return t.reshape(B, T, H, D).permute(0, 2, 1, 3)


def _live(mask, B, T, dev):
    if mask is None:
        return torch.ones((B, T), dtype=torch.bool, device=dev)
    return mask.to(dev).reshape(B, T) != 0


def check_text_attention(rec, dev, stats):
    """fwd_spec.check_attention restated for es_text_attn_fwd: head dimension 64, an arbitrary key mask instead of a key length, no lse.
    S = r(f32(q / 8)) r(k)^T, masked keys -> -inf, o = softmax(S) r(v), on the operands the launch received (r = round to bf16 in bf16
    mode, the identity in f32 mode).  The online softmax rounds the UNNORMALISED probabilities to bf16 (relative 2^-8 each), so per
    element  |o - spec| <= (2^-8 [f32 mode: 16 u] + G u sqrt(T) + 2 dS) (P |r(v)|),  dS = G u sqrt(64) max_j (|r(q / 8)| |r(k)|^T) the
    error of the score GEMM.  A sample without a live key must hold O = 0 exactly."""
    B, H, T, bf = rec['B'], rec['H'], rec['T'], rec['bf']
    E = H * D
    rr = _r if bf else _d
    qkv = rec['qkv'].to(dev).float()
    assert qkv.shape == (B * T, 3 * E)
    qs = rr(_heads(qkv[:, :E], B, T, H) * torch.tensor(SCALE, dtype=torch.float32, device=dev))
    ks, vs = rr(_heads(qkv[:, E:2 * E], B, T, H)), rr(_heads(qkv[:, 2 * E:], B, T, H))
    live = _live(rec.get('mask'), B, T, dev)[:, None, None, :]
    S = qs @ ks.transpose(-1, -2)
    dS = (G * U * math.sqrt(D) * (qs.abs() @ ks.abs().transpose(-1, -2)) * live).amax(-1)
    S = S.masked_fill(~live, -math.inf)
    dead = (~live.any(-1)).expand(B, H, T)
    lse = torch.logsumexp(S, -1).masked_fill(dead, 0.0)
    P = torch.where(dead[..., None], torch.zeros_like(S), torch.exp(S - lse[..., None]))
    o = P @ vs
    mag = P @ vs.abs()
    label = f'{stats.label}: text attention bf16={bf} B={B} H={H} T={T}'
    rel_p = (2.0 ** -8 if bf else 16 * U) + G * U * math.sqrt(T) + 2 * dS
    got = _heads(rec['o'].to(dev).double(), B, T, H)
    if bool(dead.any()) and not bool((got[dead] == 0).all()):
        raise AssertionError(f'{label}: a sample without a live key must get O = 0')
    stats.count['es_text_attn_fwd'] = stats.count.get('es_text_attn_fwd', 0) + 1
    return _held(label + ' o', got, o, rel_p[..., None] * mag, f'text attention o bf16={bf}', stats)


def text_attn_ref(qkv, mask, B, H, T, bf, leak=None):
    """the formula in f32 on the rounded operands (what an exact kernel would return up to f32 rounding); leak = (b, j): masked key j
    of sample b is let through"""
    E = H * D
    rr = (lambda t: t.to(torch.bfloat16).float()) if bf else (lambda t: t)
    q, k, v = (rr(_heads(qkv[:, i * E:(i + 1) * E].float() * (SCALE if i == 0 else 1.0), B, T, H)) for i in range(3))
    live = _live(mask, B, T, qkv.device).clone()
    if leak is not None:
        assert not bool(live[leak]), 'the leaked key must be a masked one'
        live[leak] = True
    S = (q.double() @ k.double().transpose(-1, -2)).masked_fill(~live[:, None, None, :], -math.inf)
    dead = ~live.any(-1)
    P = torch.softmax(S, -1)
    P = torch.where(dead[:, None, None, None], torch.zeros_like(P), P)
    o = (P @ v.double()).float()
    return o.permute(0, 2, 1, 3).reshape(B * T, E)


def position_ids(ids, pad_id, vocab):
    """RoBERTa's rule (create_position_ids_from_input_ids) after ids outside [0, vocab) have been replaced by pad_id:
    p = pad_id + (id != pad_id ? #{t' <= t : id[t'] != pad_id} : 0)  ->  (cleaned ids, positions), both int64 (B, T)"""
    ids = ids.long()
    ids = torch.where((ids >= 0) & (ids < vocab), ids, torch.full_like(ids, pad_id))
    live = (ids != pad_id).long()
    return ids, pad_id + torch.cumsum(live, 1) * live


def check_text_embed(rec, dev, stats):
    """es_text_embed_ln.  (1) The position ids the kernel used equal position_ids() EXACTLY.  (2) y against the f64 LayerNorm of the
    f64 sum z = word[id] + pos[p] + type0, with check_layernorm's bounds; there are no saved statistics to anchor to, so the errors of
    the kernel's own mean and rstd enter the bound of y:
      the kernel forms z in f32 with two additions:  |dz| <= ez = 2 u (|word| + |pos| + |type0|)  per element;
      mean:  |dm| <= G u sqrt(C) mean|z| + u |m| + mean(ez)                               (check_layernorm's bound + the input error)
      rstd:  a perturbation dz moves the standard deviation by at most rms(dz) <= rms(ez), and d rstd / rstd = -sigma dsigma rstd^2
             with sigma rstd <= 1, so  |d rstd| / rstd <= G u sqrt(C) + 4 u + rstd rms(ez)         (check_layernorm's bound + the input error)
      y = (z - m) rstd w + b:   |dy| <= |w| rstd (ez + |dm|) + |t| (|d rstd| / rstd) + 8 u (|t| + |b|),   t = (z - m) rstd w."""
    ids = rec['ids'].to(dev)
    B, T = ids.shape
    pad, vocab, eps = rec['pad_id'], rec['vocab'], rec['eps']
    word, pos, typ = _d(rec['word'].to(dev)), _d(rec['pos'].to(dev)), _d(rec['type0'].to(dev)).reshape(-1)
    C = word.shape[1]
    label = f'{stats.label}: text embedding B={B} T={T} C={C} eps={eps:g}'
    idc, want_p = position_ids(ids, pad, vocab)
    got_p = rec['pos_ids'].to(dev).long().reshape(B, T)
    if not torch.equal(got_p, want_p):
        bad = torch.nonzero(got_p != want_p)[0].tolist()
        raise AssertionError(f'{label}: position id at (b, t) = {tuple(bad)} is {int(got_p[tuple(bad)])}, the rule gives {int(want_p[tuple(bad)])}')
    wr, pr = word[idc.reshape(-1)], pos[want_p.reshape(-1)]
    z = wr + pr + typ[None]
    ez = 2 * U * (wr.abs() + pr.abs() + typ.abs()[None])
    m = z.mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(((z - m) ** 2).mean(1, keepdim=True) + eps)
    w, b = _d(rec['w'].to(dev))[None], _d(rec['b'].to(dev))[None]
    t = (z - m) * rs * w
    dm = G * U * math.sqrt(C) * z.abs().mean(1, keepdim=True) + U * m.abs() + ez.mean(1, keepdim=True)
    drs = G * U * math.sqrt(C) + 4 * U + rs * torch.sqrt((ez ** 2).mean(1, keepdim=True))
    bound = w.abs() * rs * (ez + dm) + t.abs() * drs + 8 * U * (t.abs() + b.abs())
    stats.count['es_text_embed_ln'] = stats.count.get('es_text_embed_ln', 0) + 1
    return _held(label + ' y', rec['y'].to(dev), t + b, bound, 'text embedding y', stats)


def embed_ref(ids, pad_id, vocab, word, pos, type0, w, b, eps):
    """f32 evaluation -> (y (B T, C), position ids (B T) int32)"""
    idc, p = position_ids(ids, pad_id, vocab)
    z = (word[idc.reshape(-1)] + pos[p.reshape(-1)]) + type0.reshape(1, -1)
    y = torch.nn.functional.layer_norm(z.double(), (z.shape[1],), w.double(), b.double(), eps).float()
    return y, p.reshape(-1).to(torch.int32)


def check_bias_gelu(rec, dev, stats):
    """es_bias_gelu: y = gelu(z), z = f32(x + bias) (ONE f32 addition: the same IEEE operation here), gelu(z) = 0.5 z (1 + erf(z / sqrt 2)).
    The kernel evaluates  f32(f32(0.5 z) f32(1 + erff(f32(z c)))),  c = f32(1 / sqrt 2):
      t = f32(z c) carries two relative roundings (c itself, the product): |d erf| <= erf'(t) |t| 2 u <= (2 / sqrt pi) max(t e^{-t^2}) 2 u < 1 u;
      erff is held to 4 u absolute;  the sum 1 + erf lies in [0, 2]: its rounding is at most 2 u;  0.5 z is exact;
      the final product adds u |y|.   =>   |dy| <= 0.5 |z| 7 u + 2 u |y|   (the second u of |y| covers the second-order terms)."""
    x, bias = rec['x'].to(dev).float(), rec['bias'].to(dev).float()
    z = (x + bias[None]).double()
    want = 0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))
    label = f'{stats.label}: bias + GELU rows {x.shape[0]} C={x.shape[1]}'
    stats.count['es_bias_gelu'] = stats.count.get('es_bias_gelu', 0) + 1
    return _held(label, rec['y'].to(dev), want, U * (3.5 * z.abs() + 2 * want.abs()), 'bias gelu', stats)


def gelu_ref(x, bias, tanh=False):
    """the formula on z = f32(x + bias), evaluated in f64 and rounded once (torch's own f32 CPU erf is a polynomial with an absolute
    error of several u: not the yardstick); tanh: the tanh approximation instead"""
    z = (x.float() + bias.float()[None]).double()
    if tanh:
        return (0.5 * z * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (z + 0.044715 * z ** 3)))).float()
    return (0.5 * z * (1.0 + torch.erf(z / math.sqrt(2.0)))).float()
