"""SparseFeatureFusion3DGrounder (embodiedscan/models/detectors/sparse_featfusion_grounder.py:29-766) on the MI355X
kernels.  Same registry name, constructor arguments and forward(inputs, data_samples, mode) protocol.

extract_feat is the mv-3ddet feature path (2-D / 3-D backbones + projection fusion, inherited) followed by MinkNeck;
pre_decoder / forward_decoder / the head run on padded channels-last token matrices.  Text: see embodiedscan_amd/text.py."""
import contextlib
import os
import torch
from ... import engine as E
from ... import hip
from ...hip import P, call
from ...params import grounder_specs
from ...registry import MODELS
from ...text import HashTokenizer, HipTextEncoder, TextGraph, build_text_encoder, create_positive_map
from ..layers.ground_transformer.decoder import SparseFeatureFusionTransformerDecoder, _Lin
from .sparse_featfusion_single_stage import SparseFeatureFusionSingleStage3DDetector

TEXT_GRAPH = [os.environ.get('ES_TEXT_GRAPH', '1') != '0']     # ... as a captured graph per token shape (text.TextGraph)
TEXT_ASYNC = [os.environ.get('ES_TEXT_ASYNC', '1') != '0']     # round 6: the frozen text encoder on its own stream, queued before the backbones


class SceneEncoding:
    """One scan encoded once (encode_scene / scene_from_tokens): everything of the grounder that does not depend on the prompt.
    feats (L, E) / points (L, 3): the MinkNeck tokens; keys: the decoder's prepared key side, one engine.PreparedKV per layer;
    precision / weight_version: engine.PRECISION[0] / engine.WEIGHT_VERSION[0] when it was built -- ground() refuses the encoding once
    either has moved (the cached projections are stale then)."""
    __slots__ = ('feats', 'points', 'L', 'keys', 'precision', 'weight_version')

    def __init__(self, feats, points, keys, precision, weight_version):
        self.feats, self.points, self.L, self.keys = feats, points, int(feats.shape[0]), keys
        self.precision, self.weight_version = precision, weight_version


class _Prompt:
    """what start_text / finish_text / bbox_head.predict read of a data sample"""

    def __init__(self, text, tokens_positive):
        import types
        # (no spans given: one target on the first character -- the positive maps do not enter the prediction)
        self.text, self.tokens_positive = text, tokens_positive if tokens_positive is not None else [[(0, 1)]]
        self.gt_instances_3d = types.SimpleNamespace()


class _TextFeatMap:
    """text_feat_map as a child of the bind bracket: the linear layer is made over the arena where it is bound"""

    def bind(self, arena, prefix):
        self.lin = _Lin(arena, prefix + 'weight', prefix + 'bias')

    def __call__(self, x, need_dx=True):
        return self.lin(x, need_dx=need_dx)


@MODELS.register_module()
class SparseFeatureFusion3DGrounder(SparseFeatureFusionSingleStage3DDetector):
    task = 'ground'

    def __init__(self, backbone, backbone_3d, bbox_head, neck=None, neck_3d=None, decoder=None, voxel_size=0.01,
                 num_queries=512, max_num_entities=256, coord_type='CAMERA', train_cfg=None, test_cfg=None,
                 data_preprocessor=None, use_xyz_feat=False, init_cfg=None, seed=0, device='cuda:0', text_encoder_cfg=None,
                 tokenizer=None, text_encoder_impl=None):
        assert neck is None and neck_3d is not None and decoder is not None
        self.backbone = MODELS.build(backbone)
        self.backbone.act16 = True              # feature maps only feed the projection fusion: bf16 activation storage
        self.backbone_3d = MODELS.build(backbone_3d)
        self.neck_3d = MODELS.build(neck_3d)
        bbox_head = dict(bbox_head)
        bbox_head.update(train_cfg=train_cfg, test_cfg=test_cfg)
        self.bbox_head = MODELS.build(bbox_head)
        self.decoder = SparseFeatureFusionTransformerDecoder(**decoder)
        self.embed_dims = self.decoder.embed_dims
        self.coord_type, self.train_cfg, self.test_cfg = coord_type, train_cfg, test_cfg
        self.num_queries = num_queries
        self.max_num_entities = self.bbox_head.contrastive_cfg.get('max_text_len', max_num_entities)
        self.voxel_size, self.use_xyz_feat = voxel_size, use_xyz_feat
        # text side (roberta-base vocabulary / weights are not available offline: stand-ins, see text.py)
        self.tokenizer = tokenizer or HashTokenizer()
        # 'torch': transformers' module, run by torch; 'hip': the same seeded module converted to text.HipTextEncoder and dropped (both
        # start from identical weights).  Not given: ES_TEXT_ENCODER decides, unset means 'torch'.
        self.text_encoder_impl = text_encoder_impl or os.environ.get('ES_TEXT_ENCODER') or 'torch'
        if self.text_encoder_impl not in ('torch', 'hip'):
            raise ValueError(f"text_encoder_impl must be 'torch' or 'hip', got {self.text_encoder_impl!r}")
        self.text_encoder = build_text_encoder(text_encoder_cfg, seed=seed)
        if self.text_encoder_impl == 'hip':
            self.text_encoder = HipTextEncoder.from_module(self.text_encoder)
        self.text_dim = self.text_encoder.config.hidden_size
        self.text_feat_map = _TextFeatMap()
        self._init_base(grounder_specs(text_dim=self.text_dim, E=self.embed_dims, num_layers=self.decoder.num_layers,
                                       ffn=self.decoder.ffn_channels, in_channels=self.neck_3d.in_channels), device, seed, data_preprocessor)

    # gradient buckets (data parallel): the backbones, the MinkNeck, and -- implicit last part -- decoder + head +
    # text_feat_map, whose gradients are complete first: four all-reduces, each under the backward of what precedes it
    _bucket_groups = (('backbone.',), ('backbone_3d.',), ('neck_3d.',))

    # ------------------------------------------------------------------ parameters
    def to(self, device):
        super().to(device)
        self.text_encoder.to(self.device)
        return self

    def _children(self):
        return [(self.backbone, 'backbone.'), (self.backbone_3d, 'backbone_3d.'), (self.neck_3d, 'neck_3d.'),
                (self.decoder, 'decoder.'), (self.bbox_head, 'bbox_head.'), (self.text_feat_map, 'text_feat_map.')]

    def _bind(self):
        if not self._bound and next(self.text_encoder.parameters()).device != self.device:
            self.text_encoder.to(self.device)
        super()._bind()

    # The frozen RoBERTa is a submodule of the reference detector, so its weights are part of the reference's state dict
    # (`text_encoder.*`, sparse_featfusion_grounder.py:104-116): a checkpoint written here must carry them and a reference
    # grounding checkpoint must load them -- otherwise the prompts would be encoded by random weights (round-2 advisor).
    def state_dict(self):
        sd = super().state_dict()
        for k, v in self.text_encoder.state_dict().items():
            sd['text_encoder.' + k] = v
        return sd

    def load_state_dict(self, sd, strict=False, tap_order=None):
        pre = 'text_encoder.'
        text = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        rest = {k: v for k, v in sd.items() if not k.startswith(pre)}
        missing, unexpected = super().load_state_dict(rest, strict=False, tap_order=tap_order)
        own = self.text_encoder.state_dict()
        dev = next(self.text_encoder.parameters()).device
        with torch.no_grad():
            for k, v in text.items():
                if k in own and tuple(own[k].shape) == tuple(v.shape):
                    own[k].copy_(v.to(dev))
                else:
                    unexpected.append(pre + k)
        # (buffers such as embeddings.position_ids exist or not depending on the transformers version: never "missing")
        params = {k for k, _ in self.text_encoder.named_parameters()}
        missing = list(missing) + [pre + k for k in own if k not in text and k in params]
        if self.text_encoder_impl == 'hip':
            self.text_encoder.refresh()          # the fused / bf16 kernel-layout copies follow the loaded weights
        if strict and (missing or unexpected):
            raise RuntimeError(f'load_state_dict: missing {missing[:5]}... unexpected {unexpected[:5]}...')
        return missing, unexpected

    # ------------------------------------------------------------------ text
    def start_text(self, batch_data_samples):
        """:475-481, first half of encode_text: tokenise, positive maps, frozen RoBERTa.  The encoder depends on the prompts only, so it is
        queued on its OWN stream before the backbones (round 6: its ~ 300 small launches used to sit between the neck and the decoder
        on the main stream, 4.6 ms of a 52.6 ms step); finish_text() joins.  ES_TEXT_ASYNC=0: on the calling stream, as before."""
        texts = [ds.text for ds in batch_data_samples]
        tok = self.tokenizer.batch_encode_plus(texts, padding='longest', return_tensors='pt')
        if all(getattr(ds, 'tokens_positive', None) is not None for ds in batch_data_samples):
            tps = [ds.tokens_positive for ds in batch_data_samples]
        else:
            tps = [[[0, 1]] for _ in batch_data_samples]
        pmaps = [create_positive_map(tok, tp, i, self.max_num_entities) for i, tp in enumerate(tps)]
        side = TEXT_ASYNC[0] and self.device.type == 'cuda'
        ev = None
        if side:
            if getattr(self, '_text_stream', None) is None:
                # the weight-gradient stream of the compute stream (idle during the forward pass) unless told otherwise: a stream of its
                # own is a fifth .. seventh stream on four hardware queues (ES_TEXT_STREAM=own: A/B)
                own = os.environ.get('ES_TEXT_STREAM', 'wgrad') == 'own' or not E.WGRAD_ASYNC[0]
                self._text_stream = torch.cuda.Stream(device=self.device) if own else E.wgrad_stream_obj()
            ctx = torch.cuda.stream(self._text_stream)
        else:
            import contextlib
            ctx = contextlib.nullcontext()
        with ctx:
            tok = tok.to(self.device)
            with torch.no_grad():
                B, T = tok.input_ids.shape
                if self.text_encoder_impl == 'hip':      # any (B, T) on the same ~ 100 launches: no graph, no shape cache
                    hs = self.text_encoder(tok.input_ids, tok.attention_mask)
                else:
                    hs = self._encode_graph(tok, B, T) if (side and TEXT_GRAPH[0]) else None
                if hs is None:
                    hs = self.text_encoder(input_ids=tok.input_ids, attention_mask=tok.attention_mask).last_hidden_state
                hs32 = hs.reshape(B * T, self.text_dim).float().contiguous()
                tlen = tok.attention_mask.sum(1).to(torch.int32).contiguous()
                mask = tok.attention_mask.bool()
            if side:
                ev = torch.cuda.Event()
                ev.record(self._text_stream)
        return dict(tok=tok, pmaps=pmaps, hs=hs, hs32=hs32, tlen=tlen, mask=mask, ev=ev, B=B, T=T)

    def _encode_graph(self, tok, B, T):
        """the frozen encoder as a graph replay per (B, T) token shape (text.TextGraph); None: this shape runs eagerly (capture failed once,
        or more than 16 shapes are alive).  Called with the text stream current."""
        graphs = self.__dict__.setdefault('_text_graphs', {})
        g = graphs.get((B, T))
        if g is None and len(graphs) < 16:
            try:
                g = TextGraph(self.text_encoder, B, T, self.device, self._text_stream)
            except Exception as exc:            # (a capture the libraries underneath do not allow: keep the eager path, say so once)
                import warnings
                warnings.warn(f'text encoder graph capture failed for shape {(B, T)}: {exc!r}; running eagerly')
                torch.cuda.synchronize(self.device)
                g = False
            graphs[(B, T)] = g
        if not g:
            return None
        return g.run(tok.input_ids, tok.attention_mask).clone()

    def finish_text(self, job, batch_data_samples):
        """:482-498, second half: the calling stream waits for the encoder, then text_feat_map (trainable, recorded on the tape HERE)"""
        if job['ev'] is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(job['ev'])
            for t in (job['hs'], job['hs32'], job['tlen'], job['mask'], job['tok'].input_ids, job['tok'].attention_mask):
                t.record_stream(cur)             # allocated on the text stream, read on this one
        mask, B, T = job['mask'], job['B'], job['T']
        for i, ds in enumerate(batch_data_samples):
            pm = job['pmaps'][i].bool().float()
            ds.gt_instances_3d.positive_maps = pm
            ds.gt_instances_3d.text_token_mask = mask[i].unsqueeze(0).repeat(len(pm), 1)
        text = self.text_feat_map(E.Var(job['hs32'], rg=False), need_dx=False)
        self.last_text = dict(hidden=job['hs'], mask=mask, input_ids=job['tok'].input_ids)
        return text, mask, job['tlen'], T

    def encode_text(self, batch_data_samples):
        """:475-498: tokenise, positive maps, frozen RoBERTa, text_feat_map.  Returns (text Var (B*T, E), mask (B,T) bool
        on the device, tlen (B,) int32 on the device, T) and attaches positive_maps / text_token_mask to the samples."""
        return self.finish_text(self.start_text(batch_data_samples), batch_data_samples)

    # ------------------------------------------------------------------ features
    def extract_feat(self, batch_inputs_dict, batch_data_samples):
        """:176-310: fused sparse levels (inherited) -> MinkNeck -> (feats, scores, coords) per-sample lists"""
        x = super().extract_feat(batch_inputs_dict, batch_data_samples)
        out = self.neck_3d(x, len(batch_data_samples))
        # everything recorded from here on (text map, decoder, head) belongs to the last gradient part (3); once the reverse
        # replay is back here only fusion + neck closures remain before the 3-D backbone's: part 2 (neck_3d.) is theirs
        self.tape_part(3)
        return out

    def forward_transformer(self, text, tlen, T, batch_data_samples):
        """pre_decoder + forward_decoder (:312-447) on the padded buffers of the neck"""
        nk = self.neck_3d.last
        feats, coords, lens, Lmax = nk['feats'], nk['points'], nk['lens'], nk['Lmax']
        B = len(lens)
        dev = feats.d.device
        s = hip.stream()
        klen = torch.tensor(lens, dtype=torch.int32).to(dev, non_blocking=True)
        # query selection: ContrastiveEmbed scores of every point token, max over text tokens, top-k per sample
        _, rowmax = self.bbox_head.cls_branch(feats, text, B, Lmax, T, tlen, vlen=klen, want_logits=False, want_max=True)
        Q = min(self.num_queries, min(lens))
        idx = torch.empty((B, Q), dtype=torch.int32, device=dev)
        call('es_topk_sorted', P(rowmax), B, Lmax, P(klen), Q, P(idx), s)
        if getattr(self, 'force_queries', None) is not None:
            # test hook (teacher forcing, tests/test_gpu_grounding.py): take the oracle's query indices so that a bf16 run can be
            # compared with its specification element by element even when the top-k boundary would flip a near tie
            self.free_queries = idx
            idx = self.force_queries.to(device=dev, dtype=torch.int32).reshape(B, Q).contiguous()
        gidx = (idx + (torch.arange(B, device=dev, dtype=torch.int32) * Lmax)[:, None]).reshape(-1).contiguous()
        query = E.gather_rows(feats, gidx)
        qcoords = torch.empty((B * Q, 3), dtype=torch.float32, device=dev)
        call('es_row_move', P(qcoords), 3, P(coords), 3, P(gidx), B * Q, 3, 0, s)
        with E.no_tape():                        # proposals: reg_branches[num_layers] on the selected tokens, detached
            pred0 = self.bbox_head.decode(qcoords, self.bbox_head.reg_branch(E.Var(query.d, rg=False))).d
        self.last_queries = dict(idx=idx, gidx=gidx, rowmax=rowmax, pred0=pred0, Q=Q, klen=klen)
        return self.decoder(query, feats, coords, qcoords, pred0, text, B, Q, Lmax, T, klen, tlen, self.bbox_head)

    # ------------------------------------------------------------------ reference protocol
    def loss(self, batch_inputs_dict, batch_data_samples, **kwargs):
        self._bind()
        job = self.start_text(batch_data_samples)
        self.extract_feat(batch_inputs_dict, batch_data_samples)
        E.mark('A19 MinkNeck (+ pruning, token padding)')
        text, mask, tlen, T = self.finish_text(job, batch_data_samples)
        E.mark('A19 frozen text encoder + text_feat_map')
        hidden, boxes = self.forward_transformer(text, tlen, T, batch_data_samples)
        E.mark('A19 query selection + 6-layer decoder')
        out = self.bbox_head.loss(hidden, boxes, text, mask, batch_data_samples, tlen=tlen)
        E.mark('A19/N2 head: token logits + Hungarian + focal + corner-Chamfer')
        return out

    def predict(self, batch_inputs_dict, batch_data_samples, **kwargs):
        with self._predict_guard():
            self._bind()
            job = self.start_text(batch_data_samples)
            self.extract_feat(batch_inputs_dict, batch_data_samples)
            text, mask, tlen, T = self.finish_text(job, batch_data_samples)
            hidden, boxes = self.forward_transformer(text, tlen, T, batch_data_samples)
            results = self.bbox_head.predict(hidden, boxes, text, mask, batch_data_samples, tlen=tlen)
        for ds, r in zip(batch_data_samples, results):
            ds.pred_instances_3d = r
        return batch_data_samples

    # ------------------------------------------------------------------ one scene, many prompts
    @contextlib.contextmanager
    def _eval_guard(self):
        """the predict guard for the entry points that do not come through forward(): + launches on the current stream, bound"""
        with self._predict_guard():
            hip.refresh_stream()
            self._bind()
            yield

    def scene_from_tokens(self, feats, points):
        """SceneEncoding of an (L, E) / (L, 3) pair of device tensors (MinkNeck tokens of one scan, e.g. from a cache file)"""
        feats = feats.to(device=self.device, dtype=torch.float32).contiguous()
        points = points.to(device=self.device, dtype=torch.float32).contiguous()
        if feats.dim() != 2 or feats.shape[1] != self.embed_dims or tuple(points.shape) != (feats.shape[0], 3):
            raise ValueError(f'expected ({{L}}, {self.embed_dims}) features and ({{L}}, 3) points, got {tuple(feats.shape)} / {tuple(points.shape)}')
        with self._eval_guard():
            keys = self.decoder.prepare_keys(E.Var(feats, rg=False), points) if feats.shape[0] else []
        return SceneEncoding(feats, points, keys, E.PRECISION[0], E.WEIGHT_VERSION[0])

    def encode_scene(self, batch_inputs_dict, batch_data_samples):
        """one SceneEncoding per sample of the batch (the samples' text is ignored): 2-D / 3-D backbones, fusion and MinkNeck run
        HERE, once per scan; ground() then answers any number of prompts on it"""
        with self._eval_guard():
            self.extract_feat(batch_inputs_dict, batch_data_samples)
            nk = self.neck_3d.last
            Lmax = nk['Lmax']
            cut = [(nk['feats'].d[b * Lmax:b * Lmax + n].clone(), nk['points'][b * Lmax:b * Lmax + n].clone()) for b, n in enumerate(nk['lens'])]
        return [self.scene_from_tokens(f, p) for f, p in cut]

    def open_walk(self, metainfo, max_frames=50):
        """a session that takes a recording one frame at a time and answers prompts on the prefix seen so far (walk.GroundWalk):
        walk.observe(img, points, depth2img) keeps the frame, walk.ask(prompts) grounds on everything observed.  The feature maps of up
        to max_frames <= 64 frames stay on the device; ValueError above that"""
        from .walk import GroundWalk
        return GroundWalk(self, metainfo, max_frames)

    def ground(self, scene, prompts, tokens_positive=None, max_prompts=64):
        """InstanceData(bboxes_3d, scores_3d, target_scores_3d) per prompt -- what predict() attaches to a (scene, prompt) sample -- for
        any number of prompts on one encoded scene, Q = min(num_queries, L) rows each.  prompts: strings or objects with .text (and
        optionally .tokens_positive); processed in chunks of at most max_prompts."""
        from ...structures import EulerDepthInstance3DBoxes, InstanceData
        if scene.precision != E.PRECISION[0] or scene.weight_version != E.WEIGHT_VERSION[0]:
            raise ValueError(f'stale scene encoding: built under precision {scene.precision!r} / weight version {scene.weight_version}, now '
                             f'{E.PRECISION[0]!r} / {E.WEIGHT_VERSION[0]}: encode the scene again')
        if scene.feats.device != self.device:
            raise ValueError(f'the scene encoding is on {scene.feats.device}, the grounder on {self.device}')
        if max_prompts < 1:
            raise ValueError('max_prompts must be positive')
        samples = []
        for i, pr in enumerate(prompts):
            tp = tokens_positive[i] if tokens_positive is not None else getattr(pr, 'tokens_positive', None)
            samples.append(_Prompt(pr if isinstance(pr, str) else pr.text, tp))
        if not samples:
            return []
        dev, L = self.device, scene.L
        if L == 0:
            z = torch.zeros(0, dtype=torch.float32, device=dev)
            return [InstanceData(bboxes_3d=EulerDepthInstance3DBoxes(torch.zeros((0, 9), dtype=torch.float32, device=dev)), scores_3d=z,
                                 target_scores_3d=z) for _ in samples]
        Q = min(self.num_queries, L)
        force = getattr(self, 'force_queries', None)
        results, free, texts, sel = [], [], [], []
        s = hip.stream()
        with self._eval_guard():
            for c0 in range(0, len(samples), max_prompts):
                chunk = samples[c0:c0 + max_prompts]
                n = len(chunk)
                text, mask, tlen, T = self.encode_text(chunk)
                texts.append(self.last_text)
                # query selection per prompt: the scene's rows scored against every prompt's tokens, top-k of the (n, L) row maxima
                _, rowmax = self.bbox_head.cls_branch_shared(scene.feats, text, n, T, tlen)
                klen = torch.full((n,), L, dtype=torch.int32, device=dev)
                idx = torch.empty((n, Q), dtype=torch.int32, device=dev)
                call('es_topk_sorted', P(rowmax), n, L, P(klen), Q, P(idx), s)
                if force is not None:                    # test hook (teacher forcing), shape (P, Q): see forward_transformer
                    free.append(idx)
                    idx = force[c0:c0 + n].to(device=dev, dtype=torch.int32).reshape(n, Q).contiguous()
                sel.append(idx)
                gidx = idx.reshape(-1)                   # rows of the ONE scene: no per-sample offset
                query = E.gather_rows(E.Var(scene.feats, rg=False), gidx)
                qcoords = torch.empty((n * Q, 3), dtype=torch.float32, device=dev)
                call('es_row_move', P(qcoords), 3, P(scene.points), 3, P(gidx), n * Q, 3, 0, s)
                pred0 = self.bbox_head.decode(qcoords, self.bbox_head.reg_branch(E.Var(query.d, rg=False))).d
                hidden, boxes = self.decoder.forward_shared(query, scene.keys, qcoords, pred0, text, n, Q, T, tlen, self.bbox_head)
                results += self.bbox_head.predict(hidden, boxes, text, mask, chunk, tlen=tlen)
        self.last_text_chunks = texts                    # last_text of every chunk (the padded token count differs between chunks)
        self.last_queries = dict(idx=torch.cat(sel), Q=Q)
        if force is not None:
            self.free_queries = torch.cat(free)
        return results

    # ------------------------------------------------------------------ many prompts per scan on one shared scene encoding (training)
    @staticmethod
    def _shared_prompts(batch_data_samples):
        """(the S*P prompt records scan-major, P) of scan-grouped data samples (pipeline.make_shared_grounding_batch); ValueError unless
        every scan carries the same positive number of prompts"""
        flat, P_ = [], None
        for i, ds in enumerate(batch_data_samples):
            pr = getattr(ds, 'prompts', None)
            if not pr:
                raise ValueError(f'data sample {i} carries no `prompts` (see pipeline.make_shared_grounding_batch)')
            if P_ is None:
                P_ = len(pr)
            elif len(pr) != P_:
                raise ValueError(f'unequal prompts per scan: sample 0 carries {P_}, sample {i} carries {len(pr)}; loss_shared is defined '
                                 f'for equal counts only (datasets.ScanGroupedGrounding always yields them)')
            flat += list(pr)
        if P_ is None:
            raise ValueError('empty batch')
        return flat, P_

    def _shared_transformer(self, feats, coords, lens, Lmax, text, tlen, T, P_):
        """forward_transformer for S scenes x P_ prompts (sample (s, p) = block s*P_ + p of the text / query rows) without the P_ copies
        of a scene's tokens: query selection by es_contrastive_shared_fwd per scene (bit-identical to the replicated form) + es_topk_sorted,
        gather_rows_shared, decoder.forward_shared_train"""
        S = len(lens)
        dev = feats.d.device
        s = hip.stream()
        Q = min(self.num_queries, min(lens))
        idx = torch.empty((S * P_, Q), dtype=torch.int32, device=dev)
        klen = torch.tensor([n for n in lens for _ in range(P_)], dtype=torch.int32).to(dev, non_blocking=True)
        rowmaxes = []
        for sc in range(S):
            rows = feats.d[sc * Lmax:sc * Lmax + lens[sc]]
            _, rowmax = self.bbox_head.cls_branch_shared(rows, E.Var(text.d[sc * P_ * T:(sc + 1) * P_ * T], rg=False), P_, T,
                                                         tlen[sc * P_:(sc + 1) * P_])
            call('es_topk_sorted', P(rowmax), P_, lens[sc], P(klen[sc * P_:(sc + 1) * P_]), Q, P(idx[sc * P_:(sc + 1) * P_]), s)
            rowmaxes.append(rowmax)
        if getattr(self, 'force_queries', None) is not None:     # test hook (teacher forcing), shape (S*P_, Q): see forward_transformer
            self.free_queries = idx
            idx = self.force_queries.to(device=dev, dtype=torch.int32).reshape(S * P_, Q).contiguous()
        off = (torch.arange(S, device=dev, dtype=torch.int32) * Lmax).repeat_interleave(P_)
        gidx = (idx + off[:, None]).reshape(-1).contiguous()
        query = E.concat_rows([E.gather_rows_shared(feats, idx[sc * P_:(sc + 1) * P_], P_, Q, r0=sc * Lmax, L=lens[sc]) for sc in range(S)])
        qcoords = torch.empty((S * P_ * Q, 3), dtype=torch.float32, device=dev)
        call('es_row_move', P(qcoords), 3, P(coords), 3, P(gidx), S * P_ * Q, 3, 0, s)
        with E.no_tape():                        # proposals: reg_branches[num_layers] on the selected tokens, detached
            pred0 = self.bbox_head.decode(qcoords, self.bbox_head.reg_branch(E.Var(query.d, rg=False))).d
        self.last_queries = dict(idx=idx, gidx=gidx, rowmax=rowmaxes, pred0=pred0, Q=Q, klen=klen)
        return self.decoder.forward_shared_train(query, feats, coords, list(lens), Lmax, qcoords, pred0, text, S, P_, Q, T, tlen,
                                                 self.bbox_head)

    def loss_shared(self, batch_inputs_dict, batch_data_samples, **kwargs):
        """`loss` on the replicated batch -- S scans with P prompts each as the S*P samples in which scan s appears P times, scan-major --
        without the copies: one data sample per scan carrying `prompts` (P records with text, tokens_positive, gt_instances_3d).  The 2-D
        backbone, voxelisation, the sparse backbone, the fusion and MinkNeck run once per scan, forward and backward; the loss dict is built by
        the same normalisation over S*P samples and the parameter gradients are the replicated batch's up to the order of floating-point
        sums (train-mode BatchNorm included: P copies of every row change neither mean nor biased variance).  Unequal P: ValueError."""
        prompts, P_ = self._shared_prompts(batch_data_samples)   # (refused before anything is launched)
        self._bind()
        job = self.start_text(prompts)
        self.extract_feat(batch_inputs_dict, batch_data_samples)
        E.mark('A19 MinkNeck (+ pruning, token padding)')
        text, mask, tlen, T = self.finish_text(job, prompts)
        E.mark('A19 frozen text encoder + text_feat_map')
        nk = self.neck_3d.last
        hidden, boxes = self._shared_transformer(nk['feats'], nk['points'], nk['lens'], nk['Lmax'], text, tlen, T, P_)
        E.mark('A19 query selection + 6-layer decoder')
        out = self.bbox_head.loss(hidden, boxes, text, mask, prompts, tlen=tlen)
        E.mark('A19/N2 head: token logits + Hungarian + focal + corner-Chamfer')
        return out

    def loss_shared_from_tokens(self, feats, points, lens, prompts):
        """loss_shared from MinkNeck tokens (the counterpart of scene_from_tokens): feats engine.Var (S*Lmax, E) that requires a gradient
        (zero rows behind each scene's lens[s] rows), points (S*Lmax, 3), lens the S token counts, prompts the S*P records scan-major.
        The prompt side, forward and backward, without the backbones; the caller runs the tape (engine.TAPE.backward())."""
        S = len(lens)
        if S < 1 or len(prompts) % S or not prompts:
            raise ValueError(f'{len(prompts)} prompts do not divide over {S} scenes: loss_shared is defined for equal counts per scene only')
        if feats.d.shape[0] % S or feats.d.shape[1] != self.embed_dims or tuple(points.shape) != (feats.d.shape[0], 3):
            raise ValueError(f'expected (S*Lmax, {self.embed_dims}) features and (S*Lmax, 3) points, got {tuple(feats.d.shape)} / {tuple(points.shape)}')
        Lmax = feats.d.shape[0] // S
        if max(lens) > Lmax or min(lens) < 1:
            raise ValueError(f'lens {list(lens)} outside [1, Lmax = {Lmax}]')
        hip.refresh_stream()
        self._bind()
        prompts = list(prompts)
        text, mask, tlen, T = self.encode_text(prompts)
        hidden, boxes = self._shared_transformer(feats, points, list(lens), Lmax, text, tlen, T, len(prompts) // S)
        return self.bbox_head.loss(hidden, boxes, text, mask, prompts, tlen=tlen)

    def train_step_shared(self, data, optim_wrapper):
        """train_step with loss_shared: data from pipeline.make_shared_grounding_batch (one sample per scan, P prompts each)"""
        def loss_fn(inputs, samples):
            hip.refresh_stream()
            return self.loss_shared(inputs, samples)
        self._shared_prompts(data['data_samples'])               # unequal P: refused before the step touches anything
        return self._train_step(data, optim_wrapper, loss_fn)
