"""Text side of the grounder (embodiedscan/models/detectors/sparse_featfusion_grounder.py:104-116,449-510,570-630).

The reference tokenises with RobertaTokenizerFast('roberta-base') and encodes with a FROZEN RobertaModel
(lr_mult 0.0, configs/grounding/...py:197-199).  Neither the vocabulary nor the weights exist offline, so:
  * `HashTokenizer` is a deterministic stand-in with the slice of the tokenizer protocol the grounder uses (batch encode
    with padding='longest', attention mask, char_to_token) -- `<s> word word ... </s>`, ids from a CRC of the word;
    a real `RobertaTokenizerFast` instance can be passed to the detector instead;
  * the text encoder is transformers' RobertaModel with RANDOM weights (a frozen, external torch module run under
    no_grad: the one place where torch computes on this path; its output is an INPUT of the trainable `text_feat_map`);
  * `HipTextEncoder` (opt-in, `SparseFeatureFusion3DGrounder(text_encoder_impl='hip')`) is the same frozen encoder on the
    project's own kernels: the module's weights are copied once, the module is dropped ("text encoder")."""
import re
import zlib
import torch


class _Encoded:
    def __init__(self, input_ids, attention_mask, spans):
        self.input_ids, self.attention_mask, self._spans = input_ids, attention_mask, spans

    def to(self, device):
        self.input_ids, self.attention_mask = self.input_ids.to(device), self.attention_mask.to(device)
        return self

    def char_to_token(self, batch_idx, char_idx):
        for t, (a, b) in enumerate(self._spans[batch_idx]):
            if a <= char_idx < b:
                return t
        return None


class HashTokenizer:
    bos, pad, eos = 0, 1, 2

    def __init__(self, vocab_size=50265):
        self.vocab_size = vocab_size

    def batch_encode_plus(self, texts, padding='longest', return_tensors='pt'):
        ids, spans = [], []
        for t in texts:
            row, sp = [self.bos], [(-1, -1)]
            for m in re.finditer(r'\S+', t):
                row.append(3 + zlib.crc32(m.group(0).lower().encode()) % (self.vocab_size - 3))
                sp.append((m.start(), m.end()))
            row.append(self.eos)
            sp.append((-1, -1))
            ids.append(row)
            spans.append(sp)
        T = max(len(r) for r in ids)
        input_ids = torch.full((len(ids), T), self.pad, dtype=torch.long)
        mask = torch.zeros((len(ids), T), dtype=torch.long)
        for i, r in enumerate(ids):
            input_ids[i, :len(r)] = torch.tensor(r)
            mask[i, :len(r)] = 1
        return _Encoded(input_ids, mask, spans)


def build_text_encoder(cfg=None, seed=0):
    """RobertaModel(RobertaConfig(**cfg)) with random weights, eval mode, no gradients"""
    from transformers import RobertaConfig, RobertaModel
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        model = RobertaModel(RobertaConfig(**(cfg or {})), add_pooling_layer=False)
    model.eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


class _FrozenWeight:
    """a frozen Linear weight in the two kernel layouts of the row-GEMM engine, made once: d (1, Cin, Cout) f32 and its bf16
    [1][Cout][Cin] copy (what engine.Param.bf16()[1] is for a trainable kernel; never re-cast: the optimiser does not see it)"""
    __slots__ = ('d', 'g', 't')

    def __init__(self, rows):
        w = torch.cat(list(rows), 0)                      # (Cout, Cin), torch.nn.Linear's layout
        self.d, self.g = w.t().contiguous()[None], None
        self.t = w.to(torch.bfloat16).contiguous()[None]

    def bf16(self):
        return None, self.t


class _Frozen:
    __slots__ = ('d', 'g')

    def __init__(self, d):
        self.d, self.g = d.contiguous(), None


class HipTextEncoder:
    """transformers' RobertaModel (frozen, eval mode, no pooler needed) evaluated by csrc/transformer.hip and the row-GEMM engine:
    es_text_embed_ln, then per layer  fused Q/K/V GEMM -> es_text_attn_fwd -> output GEMM -> es_text_add_ln (+ residual) ->
    GEMM -> es_bias_gelu -> GEMM -> es_text_add_ln (+ residual): 8 launches per layer, the same sequence for every (B, T).
    The weights live under exactly the module's state-dict names and shapes (`state_dict()` / `load_state_dict()`); the fused and
    bf16 kernel-layout copies are derived from them by refresh(), at construction / load / to(), never per call."""

    def __init__(self, config, state, device='cpu'):
        self.config = config
        self._check(config)
        self.H, self.C, self.I = config.num_attention_heads, config.hidden_size, config.intermediate_size
        self.L, self.pad_id, self.eps = config.num_hidden_layers, int(config.pad_token_id), float(config.layer_norm_eps)
        self.device = torch.device(device)
        self._sd = {k: v.detach().clone().to(self.device) for k, v in state.items()}
        self.refresh()

    @staticmethod
    def _check(cfg):
        if cfg.hidden_act != 'gelu':
            raise ValueError(f"HipTextEncoder: hidden_act must be 'gelu' (the exact erf form of es_bias_gelu), got {cfg.hidden_act!r}")
        if getattr(cfg, 'position_embedding_type', 'absolute') != 'absolute':
            raise ValueError(f'HipTextEncoder: only absolute position embeddings, got {cfg.position_embedding_type!r}')
        if cfg.hidden_size != cfg.num_attention_heads * 64:
            raise ValueError(f'HipTextEncoder: es_text_attn_fwd has head dimension 64, got hidden_size {cfg.hidden_size} / '
                             f'{cfg.num_attention_heads} heads')
        if cfg.hidden_size > 1024:
            raise ValueError(f'HipTextEncoder: the LayerNorm kernels hold rows of up to 1024 channels, got hidden_size {cfg.hidden_size}')
        if getattr(cfg, 'add_cross_attention', False) or getattr(cfg, 'is_decoder', False):
            raise ValueError('HipTextEncoder: an encoder without cross-attention only')

    @classmethod
    def from_module(cls, module, device='cpu'):
        """copy the weights of a transformers RobertaModel; the module is not kept"""
        return cls(module.config, module.state_dict(), device)

    # ---- the slice of the torch.nn.Module protocol the grounder uses
    def state_dict(self):
        return dict(self._sd)

    def named_parameters(self):
        return [(k, v) for k, v in self._sd.items() if v.is_floating_point()]

    def parameters(self):
        return iter([v for _, v in self.named_parameters()])

    def load_state_dict(self, sd, strict=True):
        missing = [k for k in self._sd if k not in sd]
        unexpected = [k for k in sd if k not in self._sd]
        bad = [k for k in sd if k in self._sd and tuple(sd[k].shape) != tuple(self._sd[k].shape)]
        if bad or (strict and (missing or unexpected)):
            raise RuntimeError(f'HipTextEncoder.load_state_dict: missing {missing[:5]} unexpected {unexpected[:5]} shape mismatch {bad[:5]}')
        with torch.no_grad():
            for k, v in sd.items():
                if k in self._sd:
                    self._sd[k].copy_(v.to(self.device))
        self.refresh()
        return missing, unexpected

    def to(self, device):
        device = torch.device(device)
        if device != self.device:
            self.device = device
            self._sd = {k: v.to(device) for k, v in self._sd.items()}
            self.refresh()
        return self

    def eval(self):
        return self

    def refresh(self):
        """re-derive the kernel-layout copies (fused Q/K/V, transposed f32, bf16) from the named weights"""
        sd = self._sd
        e = 'embeddings.'
        self._emb = tuple(sd[e + k].contiguous() for k in ('word_embeddings.weight', 'position_embeddings.weight', 'token_type_embeddings.weight',
                                                           'LayerNorm.weight', 'LayerNorm.bias'))
        self._layers = []
        for i in range(self.L):
            p = f'encoder.layer.{i}.'
            a = p + 'attention.self.'
            W = lambda *names: _FrozenWeight([sd[n + '.weight'] for n in names])
            Bv = lambda *names: _Frozen(torch.cat([sd[n + '.bias'] for n in names]))
            self._layers.append(dict(
                wqkv=W(a + 'query', a + 'key', a + 'value'), bqkv=Bv(a + 'query', a + 'key', a + 'value'),
                wo=W(p + 'attention.output.dense'), bo=Bv(p + 'attention.output.dense'),
                ln1=(sd[p + 'attention.output.LayerNorm.weight'].contiguous(), sd[p + 'attention.output.LayerNorm.bias'].contiguous()),
                w1=W(p + 'intermediate.dense'), b1=sd[p + 'intermediate.dense.bias'].contiguous(),
                w2=W(p + 'output.dense'), b2=Bv(p + 'output.dense'),
                ln2=(sd[p + 'output.LayerNorm.weight'].contiguous(), sd[p + 'output.LayerNorm.bias'].contiguous())))

    def __call__(self, input_ids, attention_mask=None):
        """(B, T) int64 token ids (+ (B, T) key mask, 0 = masked) -> (B, T, hidden) f32, queued on the current stream"""
        from . import engine as E
        from . import hip
        from .hip import P, call
        B, T = input_ids.shape
        n, C, I, H = B * T, self.C, self.I, self.H
        cur = torch.cuda.current_stream(self.device)
        st = cur.cuda_stream
        # the engine queues on hip.stream() (cached): point it at the stream that is current HERE for the length of this call
        saved = (hip._STREAM[0], hip._STREAM_OBJ[0], E.TAPE.enabled)
        hip._STREAM[0], hip._STREAM_OBJ[0], E.TAPE.enabled = st, cur, False        # frozen: nothing to differentiate
        try:
            bf = 1 if E.PRECISION[0] == 'bf16' else 0
            ids = input_ids.to(torch.int64).contiguous()
            mask = None if attention_mask is None else attention_mask.to(torch.int32).contiguous()
            word, pos, typ, lw, lb = self._emb
            x = torch.empty((n, C), dtype=torch.float32, device=ids.device)
            call('es_text_embed_ln', P(ids), B, T, self.pad_id, P(word), P(pos), P(typ), C, word.shape[0], pos.shape[0], P(lw), P(lb),
                 self.eps, P(x), 0, st)
            for ly in self._layers:
                qkv = E.linear(E.Var(x, rg=False), ly['wqkv'], ly['bqkv'], need_dx=False).d
                a = torch.empty((n, C), dtype=torch.float32, device=ids.device)
                call('es_text_attn_fwd', P(qkv), 3 * C, B, H, T, P(mask), P(a), C, bf, st)
                o = E.linear(E.Var(a, rg=False), ly['wo'], ly['bo'], need_dx=False).d
                call('es_text_add_ln', P(o), P(x), n, C, P(ly['ln1'][0]), P(ly['ln1'][1]), self.eps, P(o), st)
                h = E.linear(E.Var(o, rg=False), ly['w1'], None, need_dx=False).d
                call('es_bias_gelu', P(h), I, n, I, P(ly['b1']), st)
                x = E.linear(E.Var(h, rg=False), ly['w2'], ly['b2'], need_dx=False).d
                call('es_text_add_ln', P(x), P(o), n, C, P(ly['ln2'][0]), P(ly['ln2'][1]), self.eps, P(x), st)
        finally:
            hip._STREAM[0], hip._STREAM_OBJ[0], E.TAPE.enabled = saved
        return x.view(B, T, C)


class TextGraph:
    """The frozen encoder's forward for one (B, T) token shape as a captured HIP graph (round 6).  In eager mode the module issues ~ 300
    small launches per call from Python (4.6 ms of a 52 ms grounding step, most of it launch gaps); the weights are frozen and the module
    is in eval mode, so the launch sequence of a shape never changes: captured once on the text stream after a warm-up call, replayed
    afterwards with the token ids / mask copied into the graph's input buffers.  run() must be called with the capture stream current;
    it returns the graph's OUTPUT BUFFER (overwritten by the next replay: the caller copies what it keeps, on the same stream)."""

    def __init__(self, encoder, B, T, device, stream):
        self.ids = torch.ones((B, T), dtype=torch.long, device=device)
        self.mask = torch.ones((B, T), dtype=torch.long, device=device)
        with torch.cuda.stream(stream), torch.no_grad():
            for _ in range(2):                  # warm-up: library handles / workspaces are created outside the capture
                encoder(input_ids=self.ids, attention_mask=self.mask)
        stream.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        # (thread-local capture errors: a loader / feeder thread pinning memory while the capture runs must not invalidate it)
        with torch.no_grad(), torch.cuda.graph(self.graph, stream=stream, capture_error_mode='thread_local'):
            self.out = encoder(input_ids=self.ids, attention_mask=self.mask).last_hidden_state

    def run(self, ids, mask):
        self.ids.copy_(ids, non_blocking=True)
        self.mask.copy_(mask, non_blocking=True)
        self.graph.replay()
        return self.out


def create_positive_map(tokenized, tokens_positive, batch_idx, max_num_entities=256):
    """sparse_featfusion_grounder.py:570-621"""
    positive_map = torch.zeros((len(tokens_positive), max_num_entities), dtype=torch.float)
    for j, tok_list in enumerate(tokens_positive):
        for (beg, end) in tok_list:
            beg_pos = tokenized.char_to_token(batch_idx, beg)
            end_pos = tokenized.char_to_token(batch_idx, end - 1)
            if beg_pos is None:
                beg_pos = tokenized.char_to_token(batch_idx, beg + 1)
                if beg_pos is None:
                    beg_pos = tokenized.char_to_token(batch_idx, beg + 2)
            if end_pos is None:
                end_pos = tokenized.char_to_token(batch_idx, end - 2)
                if end_pos is None:
                    end_pos = tokenized.char_to_token(batch_idx, end - 3)
            if beg_pos is None or end_pos is None:
                continue
            positive_map[j, beg_pos:end_pos + 1].fill_(1)
    return positive_map / (positive_map.sum(-1)[:, None] + 1e-6)
