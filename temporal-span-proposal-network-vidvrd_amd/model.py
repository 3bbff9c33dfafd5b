"""Drop-in `BaseModel` for the TSPN relation-scoring hot path on MI355X.

Mirrors the reference's module tree so that `BaseModel(cfg)`, `forward(pair_list,
target_list)`, the return conventions and the `state_dict` key names are the same
(reference lib/modeling/model.py:7-88, relpn/relpn.py:9-60, relpn/ppn.py:7-112,
relpn/dpn.py:9-81), while every tensor operation of the eval
forward runs in the hand-written HIP library (ops.py -> C ABI).  The nn.Linear /
nn.Conv1d objects below are parameter holders only; their own forward is never
called.

Differences from the reference, all in code the reference cannot execute:
  * USE_DPN=True: the reference raises NameError (relpn/dpn.py:24-28).  Here the
    temporal branch runs: pair builder -> temporal encoder -> relationness +
    span-regression heads, RelOIPool over the segment, predicate head
    (semantics frozen in DESIGN.md §2); in train mode it returns the loss the
    reference intended (`loss_duration`, relpn/dpn.py:40-49).
  * `relness_pred` (relpn/dpn_anchor.py:88-90) is an extra parameter; reference
    checkpoints that lack it still load (see DPNHead._load_from_state_dict).
There is no CPU execution path: without the HIP library or a HIP device,
forward raises.
"""
import contextlib
import functools
import warnings
import weakref
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _abi, hashrng, ops
from .sampler import BalancedPositiveNegativePairSampler

TemporalProposals = namedtuple("TemporalProposals", ["relness", "duration", "heads", "geom"], defaults=[None])
TemporalProposals.__doc__ = """Per-segment output of the temporal branch:
relness [P,A,T] relationness logits, duration [P,2A,T] span regression (views of heads [P,3A,T]);
geom [P,8,T]: the bbox half of the pair builder (relative box geometry per pair and frame, DESIGN.md §2) when
the segment carries 'tracklet_boxes', else None."""


def _compute_device(*tensors):
    """Device the HIP path runs on: that of the first HIP tensor seen, else the current HIP device."""
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    if not torch.cuda.is_available():
        raise RuntimeError("TSPN BaseModel: no HIP device available; this build has no CPU path "
                           "(the reference's CPU forward is restated only as the test oracle)")
    return torch.device("cuda", torch.cuda.current_device())


def invalidate_caches(module):
    """Drop every packed / device-resident weight copy held under `module` (see _DeviceCache)."""
    for m in module.modules():
        for cache in vars(m).values():
            if isinstance(cache, _DeviceCache):
                cache.clear()
        if hasattr(m, "_logits_token"):
            m._logits_token = None       # never let a decode ride the ready-event of a pass made with other weights


class _CachedWeightsMixin:
    """nn.Module mix-in: anything that can replace parameter values wholesale clears the weight caches."""

    def invalidate_caches(self):
        invalidate_caches(self)

    def train(self, mode=True):
        invalidate_caches(self)
        return super().train(mode)

    def _apply(self, fn, *args, **kwargs):
        invalidate_caches(self)
        return super()._apply(fn, *args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        invalidate_caches(self)
        return super().load_state_dict(*args, **kwargs)


def _f32(t, device):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(t)
    return t.to(device=device, dtype=torch.float32).contiguous()


def _consecutive_view(tensors):
    """Zero-copy batch of equal-shape tensors that already lie back to back in ONE allocation (the slices
    `big[b*N:(b+1)*N]` of a batched tensor a loader handed out per segment): the [len * rows, ...] view of that
    allocation, or None when the tensors are not laid out that way."""
    t0 = tensors[0]
    if not isinstance(t0, torch.Tensor) or t0.dim() == 0 or not t0.is_contiguous():
        return None
    step = t0.numel() * t0.element_size()
    base = t0.untyped_storage().data_ptr()
    for k, t in enumerate(tensors):
        if (not isinstance(t, torch.Tensor) or t.shape != t0.shape or t.dtype != t0.dtype or t.device != t0.device
                or not t.is_contiguous() or t.data_ptr() != t0.data_ptr() + k * step
                or t.untyped_storage().data_ptr() != base):
            return None
    if t0.storage_offset() * t0.element_size() + len(tensors) * step > t0.untyped_storage().nbytes():
        return None
    return torch.as_strided(t0, (len(tensors) * t0.shape[0],) + tuple(t0.shape[1:]), t0.stride())


def _batch_rows(tensors, device, dtype=torch.float32):
    """cat(tensors) on `device` as `dtype` — without the copy when they are consecutive slices of one tensor."""
    t0 = tensors[0]
    if isinstance(t0, torch.Tensor) and t0.device == device and t0.dtype == dtype:
        v = _consecutive_view(tensors)
        if v is not None:
            return v
    conv = []
    for t in tensors:
        if isinstance(t, np.ndarray):
            t = torch.from_numpy(t)
        conv.append(t.to(device=device, dtype=dtype).contiguous())
    return conv[0] if len(conv) == 1 else torch.cat(conv)


def _pairs_field(plist):
    """A segment's 'tracklet_pairs' field as an int64 tensor on the device it lives on (no copy between devices: every
    caller moves it where it validates or reads it), or None when the segment scores all ordered pairs."""
    p = plist.get_field("tracklet_pairs") if plist.has_field("tracklet_pairs") else None
    if p is None:
        return None
    return (p.detach() if isinstance(p, torch.Tensor) else torch.as_tensor(np.asarray(p))).long()


def _have_boxes(pair_list, members, on_device=False):
    """Every member carries 'tracklet_boxes' (`on_device`: as HIP tensors, which the side stream may read in place)."""
    boxes = [pair_list[i].get_field("tracklet_boxes") if pair_list[i].has_field("tracklet_boxes") else None for i in members]
    if on_device:
        return all(isinstance(b, torch.Tensor) and b.is_cuda for b in boxes)
    return all(b is not None for b in boxes)


def _segment_pairs(plist, n, device):
    """int64 [P,2] pair table of a tracklet segment: its 'tracklet_pairs' field or all ordered pairs."""
    p = _pairs_field(plist)
    if p is not None:
        p = p.to(device)
        if p.dim() != 2 or p.shape[1] != 2:
            raise ValueError("tracklet_pairs must be [P,2]")
        if p.numel() and (int(p.min()) < 0 or int(p.max()) >= n):
            raise IndexError("tracklet_pairs index out of range")
        return p.contiguous()
    return ops.pair_index(n, device)


_VERIFY_WEIGHTS = __import__("os").environ.get("TSPN_VERIFY_WEIGHTS", "0") not in ("", "0")


class _DeviceCache:
    """Device-resident (and packed) copies of parameters, refreshed when a parameter changes.

    Contract: a change is seen through the parameter's storage pointer, its autograd version counter and
    its device — optimiser steps, `load_state_dict`, `.to()` / `.cuda()` and `train()` all refresh the
    cache (the last three through `invalidate_caches`).  In-place edits through `.data` (`p.data.copy_`,
    EMA updates, legacy loaders) bump none of these: call `model.invalidate_caches()` after them, or run with
    TSPN_VERIFY_WEIGHTS=1 (a content fingerprint per parameter and forward: safe with any training loop, slower)."""

    def __init__(self):
        self._store = {}

    def get(self, key, params, device, build):
        sig = tuple((p.data_ptr(), p._version, str(p.device)) for p in params) + (str(device),)
        if _VERIFY_WEIGHTS:
            # TSPN_VERIFY_WEIGHTS=1: a content fingerprint joins the signature, so in-place `.data` edits (EMA, legacy
            # loaders) refresh the cache too -- at the price of a device reduction and a host sync per parameter and call
            with torch.no_grad():
                sig += tuple((float(p.detach().double().sum()), float(p.detach().double().abs().sum())) for p in params)
        hit = self._store.get(key)
        if hit is not None and hit[0] == sig:
            return hit[1]
        with torch.no_grad():
            value = build([_f32(p.detach(), device) for p in params])
        self._store[key] = (sig, value)
        return value

    def clear(self):
        self._store.clear()


def _nt(a, b, bias=None, sigmoid=False):
    """a [M,K] . b [N,K]^T (+ bias [N]) on the HIP split-K MFMA GEMM of the predicate head (tspn_predicate_head_f32): the
    one GEMM form the library has, so every product of the training step is brought to it with HIP transposes."""
    m, k = a.shape
    n = b.shape[0]
    if m == 0 or n == 0 or k == 0:
        # an empty product (no sampled pairs / an empty batch): the sum over nothing is zero -- the C entry refuses
        # zero-length contractions, the reference's torch.mm / einsum return zeros (and zero gradients) here
        out = torch.zeros((m, n), dtype=torch.float32, device=a.device)
        if bias is not None:
            out = out + bias
        return torch.sigmoid(out) if sigmoid else out
    return ops.predicate_head(a.contiguous(), b.contiguous(), None if bias is None else bias.contiguous(), apply_sigmoid=sigmoid)


def _tr(a):
    """[M,N] -> [N,M] contiguous (tspn_transpose_td_f32)."""
    if a.numel() == 0:
        return a.new_zeros((a.shape[1], a.shape[0]))      # an empty batch: the C entry refuses zero-length axes
    return ops.transpose_td(a.contiguous().unsqueeze(0))[0]


def _col_sums(g):
    """Column sums of g [M,N], rows added in order (tspn_temporal_sum_f32): the bias gradients; zero for an empty batch."""
    if g.shape[0] == 0:
        return g.new_zeros((g.shape[1],))
    return ops.temporal_sum(g.contiguous().unsqueeze(0))[0]


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b with HIP forward AND backward (round 4; the backward was torch / rocBLAS GEMMs before):
        dx = g W = nt(g, W^T),   dW = g^T x = nt(g^T, x^T),   db = column sums of g  (tspn_temporal_sum_f32)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        return _nt(x, w, b)

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        gx = _nt(g, _tr(w)) if ctx.needs_input_grad[0] else None
        gw = _nt(_tr(g), _tr(x)) if ctx.needs_input_grad[1] else None
        gb = _col_sums(g) if ctx.needs_input_grad[2] else None
        return gx, gw, gb


class _MatmulNTFn(torch.autograd.Function):
    """a b^T with HIP forward and backward: da = g b = nt(g, b^T), db = g^T a = nt(g^T, a^T)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return _nt(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        ga = _nt(g, _tr(b)) if ctx.needs_input_grad[0] else None
        gb = _nt(_tr(g), _tr(a)) if ctx.needs_input_grad[1] else None
        return ga, gb


class _PredicateHeadFn(torch.autograd.Function):
    """sigmoid(x W^T + b): HIP forward (sigmoid inside the GEMM's reduce kernel) and HIP backward (see _LinearFn)."""

    @staticmethod
    def forward(ctx, x, w, b):
        out = ops.predicate_head(x, w, b, apply_sigmoid=True)
        ctx.save_for_backward(x, w, out)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, out = ctx.saved_tensors
        gz = (g * out * (1.0 - out)).contiguous()
        gx = _nt(gz, _tr(w)) if ctx.needs_input_grad[0] else None
        gw = _nt(_tr(gz), _tr(x)) if ctx.needs_input_grad[1] else None
        gb = _col_sums(gz) if ctx.needs_input_grad[2] else None
        return gx, gw, gb


def _rows_of(x):
    """[R, C, T] -> [C, R*T] contiguous (a torch permute + copy: byte movement, no arithmetic)."""
    return x.permute(1, 0, 2).reshape(x.shape[1], -1).contiguous()


def _conv3_weight_grad(x_cf, dz):
    """dL/dW of y = Conv1d(k=3, padding=1)(x): W[m, c, k] = sum_{n,t} dz[n, m, t] x[n, c, t + k - 1]: per tap one product
    dZ [M, R T] . X_k [C, R T]^T on the library's HIP GEMM (round 4; three torch einsums before); x_cf [R, Cin, T], dz [R, M, T]."""
    xp = F.pad(x_cf, (1, 1))
    t = x_cf.shape[2]
    dzr = _rows_of(dz)
    return torch.stack([_nt(dzr, _rows_of(xp[:, :, k:k + t])) for k in range(3)], dim=2)


def _heads_backward(head_w, g, act):
    """Backward of heads = head_w . act (+ b) for g [P,H,T], act [P,C,T] = relu(...):
    dZ [P,C,T] = (head_w^T g) . [act > 0]  and  d_head_w [H,C] = sum_{p,t} g act -- two products on the HIP GEMM."""
    p, h, t = g.shape
    c = act.shape[1]
    gt = g.permute(0, 2, 1).reshape(p * t, h).contiguous()              # [(p,t), H]
    dz = _nt(gt, _tr(head_w)).view(p, t, c).permute(0, 2, 1) * (act > 0)  # [(p,t), C] -> [P,C,T]
    d_head_w = _nt(_rows_of(g), _rows_of(act))                          # [H, P T] . [C, P T]^T
    return dz.contiguous(), d_head_w


class _TemporalHeadsDenseFn(torch.autograd.Function):
    """DPNHead on a materialised x [P,C,T] (reference relpn/dpn.py:69-73) for training: HIP forward
    (tspn_temporal_encoder_heads_f32); backward recomputes the encoder activation with the HIP conv and forms every
    product on the library's HIP GEMM / conv kernels (round 4; torch einsums before)."""

    @staticmethod
    def forward(ctx, x, conv_w, conv_b, head_w, head_b):
        heads = ops.temporal_encoder_heads(x, ops.pack_conv3(conv_w), conv_b, head_w, head_b)
        ctx.save_for_backward(x, conv_w, conv_b, head_w)
        return heads

    @staticmethod
    def backward(ctx, g):
        x, conv_w, conv_b, head_w = ctx.saved_tensors
        g = g.contiguous()
        act = ops.conv3(x, ops.pack_conv3(conv_w), conv_b, relu=True)          # relu(conv(x) + b) [P,C,T]
        dz, d_head_w = _heads_backward(head_w, g, act)
        dx = None
        if ctx.needs_input_grad[0]:
            # conv1d_input = the k=3 conv of dZ with the taps reversed and the channel roles swapped
            dx = ops.conv3(dz, ops.pack_conv3(conv_w.flip(2).transpose(0, 1).contiguous()), None, relu=False)
        return dx, _conv3_weight_grad(x, dz), dz.sum((0, 2)), d_head_w, g.sum((0, 2))


def _tracklet_projections(feats, conv_w, conv_b):
    """U‖V [NT, 2C, T] of tracklet features [NT, T, D] on the split-packed conv weight: the channels-last
    kernel when D % 16 == 0, else what the fused eval pass does for such a D -- HIP transpose + the direct kernel -- so
    that every model that scores can also be trained."""
    d = feats.shape[2]
    packed = ops.pack_conv3(conv_w, split=d)
    bias2 = torch.cat([conv_b, torch.zeros_like(conv_b)])
    if d % 16 == 0:
        return ops.conv3_tc(feats, packed, bias2)
    return ops.conv3(ops.transpose_td(feats), packed, bias2)


class _TemporalHeadsTrackletFn(torch.autograd.Function):
    """Factorised pair encoder + heads on tracklet tensors for training.  Forward: the HIP
    projections U‖V (tspn_conv3_tc_f32 on the split-packed weight) and the indexed pair stage
    (tspn_heads_f32).  Backward: dZ_p = (head_w^T g_p) . [relu(U[s]+V[o]) > 0] per block of pairs (HIP GEMM),
    scattered back onto dU[s], dV[o]; the conv weight gradient is then a per-TRACKLET contraction (the
    same N-1 saving as the forward)."""

    PAIR_BLOCK = 256

    @staticmethod
    def forward(ctx, feats, pairs, conv_w, conv_b, head_w, head_b):
        c = 2 * feats.shape[2]
        y = _tracklet_projections(feats, conv_w, conv_b)                          # [NT, 2C, T]
        s, o = pairs[:, 0].contiguous(), pairs[:, 1].contiguous()
        heads = ops.heads(y[:, :c].contiguous(), head_w, head_b, b=y[:, c:].contiguous(), ia=s, ib=o)
        ctx.save_for_backward(feats, pairs, conv_w, conv_b, head_w)
        return heads

    @staticmethod
    def backward(ctx, g):
        feats, pairs, conv_w, conv_b, head_w = ctx.saved_tensors
        g = g.contiguous()
        c = 2 * feats.shape[2]
        y = _tracklet_projections(feats, conv_w, conv_b)
        u, v = y[:, :c], y[:, c:]
        du, dv = torch.zeros_like(u), torch.zeros_like(v)
        d_head_w = torch.zeros_like(head_w)
        for lo in range(0, pairs.shape[0], _TemporalHeadsTrackletFn.PAIR_BLOCK):
            blk = slice(lo, lo + _TemporalHeadsTrackletFn.PAIR_BLOCK)
            s, o, gb = pairs[blk, 0], pairs[blk, 1], g[blk].contiguous()
            act = torch.relu(u[s] + v[o])
            dz, dhw = _heads_backward(head_w, gb, act)
            d_head_w += dhw
            # accumulate=True takes torch's sort-based scatter: rows of one tracklet are added in a fixed order, so the
            # gradients of a step are the same bits in every run (index_add_ adds them with atomics, in any order)
            du.index_put_((s,), dz, accumulate=True)
            dv.index_put_((o,), dz, accumulate=True)
        x_cf = feats.transpose(1, 2)
        d_conv_w = torch.cat([_conv3_weight_grad(x_cf, du), _conv3_weight_grad(x_cf, dv)], dim=1)
        return None, None, d_conv_w, du.sum((0, 2)), d_head_w, g.sum((0, 2))


class _SpanLossFn(torch.autograd.Function):
    """(loss_relationness, loss_duration_proposal) of one segment from its heads [P,3A,T] and ground-truth spans
    [P,G,2]: anchor labels, both losses and their gradient in three HIP entries (ops.span_anchor_labels,
    ops.span_loss; with `sample`, ops.span_anchor_sample between them), nothing synchronised.  The forward already holds the gradient of each loss with respect to its own
    rows of the heads; the backward multiplies the two row groups by the upstream gradients."""

    @staticmethod
    def forward(ctx, heads, gt, sizes, pos_iou, neg_iou, beta, sample=None):
        heads = heads.contiguous()
        label, matched = ops.span_anchor_labels(gt, sizes, heads.shape[2], pos_iou=pos_iou, neg_iou=neg_iou)
        mask = None
        if sample is not None:                # (batch, positive_fraction, stream_key): the balanced mini-batch of this segment
            mask, _ = ops.span_anchor_sample(label, *sample)
        out, dheads = ops.span_loss(heads, gt, sizes, label, matched, mask=mask, beta=beta)
        ctx.save_for_backward(dheads)
        ctx.num_anchors = len(sizes)
        return out[0].float(), out[1].float()

    @staticmethod
    def backward(ctx, g_rel, g_reg):
        dheads, = ctx.saved_tensors
        a = ctx.num_anchors
        scale = torch.cat([g_rel.reshape(1).expand(a), g_reg.reshape(1).expand(2 * a)]).to(dheads.dtype)
        return dheads * scale.view(1, 3 * a, 1), None, None, None, None, None, None


def _span_cls_weight_grad(dG, feats):
    """dW [K,2D] of the span-pooled predicate head from dG [NT,T,2K] (ops.span_predicate_grad) and feats [NT,T,D]:
    dW[k, h D + c] = sum over (n, t) of dG[n, t, 2k + h] feats[n, t, c], one product dG^T [2K, NT T] . feats^T [D, NT T]^T on
    the library's HIP GEMM; row 2k + h of the product is half h of row k of dW."""
    nt, t, k2 = dG.shape
    d = feats.shape[2]
    return _nt(_tr(dG.reshape(nt * t, k2)), _tr(feats.reshape(nt * t, d))).reshape(k2 // 2, 2 * d)


class _SpanPredicateLossFn(torch.autograd.Function):
    """loss_rel of one shape group of tracklet segments from the predicate head pooled over each pair's ground-truth spans
    (DESIGN.md §2 "span-pooled predicate training"): feats [NT,T,D] (the group's tracklets back to back), pairs [P,2]
    global ids, the target fields spans [P,G,2] / span_count [P] / span_labels [P,G,K], pair_off [S+1] or None.  The
    forward holds d loss / d v of every row (ops.span_predicate_loss); the backward turns it into the gradients of the
    classifier (ops.span_predicate_grad and one GEMM).  The features get no gradient, as with the segment-pooled rows."""

    @staticmethod
    def forward(ctx, feats, pairs, spans, span_count, span_labels, w, b, pair_off):
        out, _, dv, _, scratch = ops.span_predicate_loss(feats, pairs, spans, span_count, span_labels, w, b,
                                                         pair_off=pair_off)
        ctx.save_for_backward(feats, pairs, spans, span_count, dv)
        ctx.scratch = scratch
        return out[0].float()

    @staticmethod
    def backward(ctx, g):
        feats, pairs, spans, span_count, dv = ctx.saved_tensors
        db, dG = ops.span_predicate_grad(dv, pairs, spans, span_count, feats.shape[0], feats.shape[1], scratch=ctx.scratch)
        gw = _span_cls_weight_grad(dG, feats) * g if ctx.needs_input_grad[5] else None
        gb = db * g if ctx.needs_input_grad[6] else None
        return None, None, None, None, None, gw, gb, None


class RelationPredictor(nn.Module):
    """Predicate-classification head (reference lib/modeling/model.py:76-88)."""

    # block-L1 layout of the 11070-d baseline feature (lib/dataset/vrdataset.py:227-236)
    PREPROCESS_BLOCKS = (70, 1000, 8)

    def __init__(self, in_channels, out_channels, fuse_preprocess=False):
        super().__init__()
        self.rel_predictor = nn.Linear(in_channels, out_channels)
        nn.init.normal_(self.rel_predictor.weight, std=0.01)
        nn.init.constant_(self.rel_predictor.bias, 0)
        # PREDICT.FUSE_PREPROCESS: features arrive RAW (the DataLoader skips _feature_preprocess) and
        # the normalisation is folded into the predicate GEMM; eval only
        self.fuse_preprocess = bool(fuse_preprocess)
        self._cache = _DeviceCache()

    def forward(self, reloi_feats):
        dev = _compute_device(reloi_feats, self.rel_predictor.weight)
        x = _f32(reloi_feats, dev)
        w, b = self.rel_predictor.weight, self.rel_predictor.bias
        if torch.is_grad_enabled() and (w.requires_grad or x.requires_grad):
            if not w.is_cuda:
                raise RuntimeError("training needs the model on the HIP device (model.cuda())")
            out = _PredicateHeadFn.apply(x, w.contiguous(), b.contiguous())
        else:
            wd, bd = self._cache.get("cls", (w, b), dev, lambda ts: ts)
            first, block, nblocks = self.PREPROCESS_BLOCKS
            norm = self.PREPROCESS_BLOCKS if (self.fuse_preprocess and x.dim() == 2
                                              and x.shape[1] >= first + block * nblocks) else None
            out = ops.predicate_head(x, wd, bd, apply_sigmoid=True, norm=norm)
        return out.to(reloi_feats.device)


class RelOIPool:
    """Relation-of-interest pooling (reference lib/modeling/model.py:68-73).

    2-D feats [P,F] pass through (duration_proposals None).  Temporal feats
    [P,C,T] are averaged over the segment (build-defined)."""

    def __call__(self, feats, duration_proposals):
        if duration_proposals is None:
            return feats
        return [ops.temporal_mean(f, layout_tc=False) if f.dim() == 3 else f for f in feats]


class PPNHead(nn.Module):
    """Tracklet-level relationness embeddings (reference lib/modeling/relpn/ppn.py:92-112)."""

    def __init__(self, in_channels, hidden_channels, out_channels):
        super().__init__()
        self.sub_emb = nn.Sequential(nn.Linear(in_channels, hidden_channels), nn.ReLU(True),
                                     nn.Linear(hidden_channels, out_channels))
        self.obj_emb = nn.Sequential(nn.Linear(in_channels, hidden_channels), nn.ReLU(True),
                                     nn.Linear(hidden_channels, out_channels))

    def weights(self):
        names = ["sub_emb.0.weight", "sub_emb.0.bias", "sub_emb.2.weight", "sub_emb.2.bias",
                 "obj_emb.0.weight", "obj_emb.0.bias", "obj_emb.2.weight", "obj_emb.2.bias"]
        sd = dict(self.named_parameters())
        return names, [sd[n] for n in names]

    def forward(self, sub_logits, obj_logits):
        """Autograd (training) form: every GEMM of the two MLPs and of the pair matrix, forward and backward, on the
        library's HIP GEMM (round 4; torch.mm before); ReLU / sigmoid are elementwise torch ops.  Eval goes through
        PPN.propose (one fused launch)."""
        def mlp(seq, x):
            h = torch.relu(_LinearFn.apply(x.contiguous(), seq[0].weight, seq[0].bias))
            return _LinearFn.apply(h, seq[2].weight, seq[2].bias)
        if not sub_logits.is_cuda:
            raise RuntimeError("training needs the inputs on the HIP device")
        s = mlp(self.sub_emb, sub_logits.float())
        o = mlp(self.obj_emb, obj_logits.float())
        return torch.sigmoid(_MatmulNTFn.apply(s, o))


class PPN(nn.Module):
    """Pair Proposal Network (reference lib/modeling/relpn/ppn.py:7-90)."""

    def __init__(self, cfg):
        super().__init__()
        self.num_pair_proposals = cfg.RELPN.PPN.NUM_PAIR_PROPOSALS
        self.ppn_head = PPNHead(cfg.RELPN.PPN.IN_CHANNELS, cfg.RELPN.PPN.HIDDEN_CHANNELS,
                                cfg.RELPN.PPN.OUT_CHANNELS)
        # the reference also constructs (and never calls) a balanced sampler: ppn.py:20-23
        self.batch_size_per_segment = cfg.RELPN.PPN.BATCH_SIZE_PER_SEGMENT
        self.positive_fraction = cfg.RELPN.PPN.POSITIVE_FRACTION
        # constructed like the reference (relpn/ppn.py:20-23); it never calls it either
        self.fg_bg_sampler = BalancedPositiveNegativePairSampler(
            batch_size_per_image=self.batch_size_per_segment, positive_fraction=self.positive_fraction)
        self._cache = _DeviceCache()

    def device_weights(self, dev):
        """Device-resident copies of the two MLPs (cached).  BaseModel calls this on the CALLER's stream before it
        sends `propose` to its side stream, so the copies are made, and their memory owned, by the caller's stream."""
        names, params = self.ppn_head.weights()
        return self._cache.get("ppn", params, dev, lambda ts: dict(zip(names, ts)))

    def propose(self, cls_logits):
        """Eval: one fused HIP launch per group of equal-N segments -> (matrices, top-k indices)."""
        _, params = self.ppn_head.weights()
        dev = _compute_device(*cls_logits, params[0])
        w = self.device_weights(dev)
        mats, idxs = [None] * len(cls_logits), [None] * len(cls_logits)
        groups = {}
        for i, c in enumerate(cls_logits):
            groups.setdefault(tuple(c.shape), []).append(i)
        for shape, members in groups.items():
            batch = _batch_rows([cls_logits[i] for i in members], dev).view((len(members),) + tuple(shape))
            mat, idx = ops.ppn_pair_matrix_topk(batch, w, self.num_pair_proposals)
            for k, i in enumerate(members):
                mats[i] = mat[k].to(cls_logits[i].device)
                idxs[i] = idx[k].to(cls_logits[i].device)
        return mats, idxs

    @staticmethod
    def _gt_matrices(pair_list, target_list):
        """N x N 0/1 matrices: 1 where any predicate is set for (s,o) (ppn.py:36-49, host side)."""
        out = []
        for plist, tlist in zip(pair_list, target_list):
            pairs = torch.as_tensor(np.asarray(plist.get_field("tracklet_pairs"))).long().cpu()
            n = int(plist.get_field("num_tracklets"))
            pos = (tlist.target.detach().sum(dim=1) > 0).cpu()
            gt = torch.zeros(n, n)
            m = min(len(pairs), len(pos))   # zip(track_pair, pred_label) stops at the shorter one (ppn.py:44)
            sel = pairs[:m][pos[:m]]
            gt[sel[:, 0], sel[:, 1]] = 1
            out.append(gt)
        return out

    def forward(self, pair_list, target_list=None):
        cls_logits = [plist.get_field("track_cls_logits") for plist in pair_list]
        if not self.training:
            _, idx = self.propose(cls_logits)
            return idx, {}
        gts = self._gt_matrices(pair_list, target_list)
        proposals, loss = [], 0
        for c, gt in zip(cls_logits, gts):
            pm = self.ppn_head(c, c)
            loss = loss + F.binary_cross_entropy(pm, gt.to(pm.device))
            order = torch.sort(pm.detach().view(-1), descending=True, stable=True)[1]
            proposals.append(order[: self.num_pair_proposals])
        return proposals, {"loss_pair": loss}


class DPNHead(nn.Module):
    """Temporal context encoder + span-regression (+ relationness) heads
    (reference lib/modeling/relpn/dpn.py:55-73; relness_pred from relpn/dpn_anchor.py:82-108)."""

    def __init__(self, in_channels, num_windows):
        super().__init__()
        self.conv = nn.Conv1d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)
        self.duration_pred = nn.Conv1d(in_channels, num_windows * 2, kernel_size=1, stride=1)
        self.relness_pred = nn.Conv1d(in_channels, num_windows, kernel_size=1, stride=1)
        for layer in (self.conv, self.duration_pred, self.relness_pred):
            nn.init.normal_(layer.weight, std=0.01)
            nn.init.constant_(layer.bias, 0)
        self.in_channels = in_channels
        self.num_windows = num_windows

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys,
                              unexpected_keys, error_msgs):
        # reference checkpoints (dpn.py) carry no relness_pred: keep the initialised values
        for leaf in ("relness_pred.weight", "relness_pred.bias"):
            if prefix + leaf not in state_dict:
                state_dict[prefix + leaf] = dict(self.named_parameters())[leaf].detach().clone()
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys,
                                      unexpected_keys, error_msgs)

    def head_params(self):
        return (self.relness_pred.weight, self.relness_pred.bias,
                self.duration_pred.weight, self.duration_pred.bias)


class DPN(nn.Module):
    """Duration Proposal Network (reference lib/modeling/relpn/dpn.py:9-52), runnable."""

    def __init__(self, cfg, in_channels, num_windows):
        super().__init__()
        self.dpn_head = DPNHead(in_channels, num_windows)
        self.top_k_proposals = cfg.RELPN.DPN.NUM_DURATION_PROPOSALS  # RelNMS stub: rel_nms.py:11
        self._cache = _DeviceCache()
        self._anchor_sizes_cfg = getattr(cfg.RELPN.DPN, "ANCHOR_SIZES", None)
        # build extension: training from ground-truth spans (target field 'spans')
        sl = getattr(cfg.RELPN.DPN, "SPAN_LOSS", None)
        self.span_pos_iou = float(getattr(sl, "POS_IOU", 0.7))
        self.span_neg_iou = float(getattr(sl, "NEG_IOU", 0.3))
        self.span_beta = float(getattr(sl, "SMOOTH_L1_BETA", 1.0 / 9.0))
        # 0 = every labelled anchor enters the losses; > 0 = a balanced mini-batch per segment, sampled on the device
        self.span_batch = int(getattr(sl, "BATCH_SIZE_PER_SEGMENT", 0))
        self.span_positive_fraction = float(getattr(sl, "POSITIVE_FRACTION", 0.5))
        self.reseed_span_sampler(int(getattr(sl, "SAMPLE_SEED", 0)))

    def reseed_span_sampler(self, seed, start=0):
        """The c-th segment sampled from here on draws its keys from stream (seed, "span_sample/{start + c}").  The
        counter is a plain attribute, not part of the state dict: a resumed run reseeds with the count it stopped at,
        and every rank of a data-parallel run takes its own seed."""
        self._span_sample_seed, self._span_sample_count = int(seed), int(start)

    def _next_span_sample(self):
        """The `sample` argument of _SpanLossFn for the next segment, or None when sampling is off."""
        if self.span_batch <= 0:
            return None
        key = hashrng.stream_key(self._span_sample_seed, f"span_sample/{self._span_sample_count}")
        self._span_sample_count += 1
        return (self.span_batch, self.span_positive_fraction, key)

    def anchor_sizes(self, num_frames):
        """Anchor widths (frames) of the A anchors per location.  cfg.RELPN.DPN.ANCHOR_SIZES when it
        is a sequence of length A; the reference ships a placeholder int there (defaults.py:66), so
        the default is the proportions of its own example (anchor_generator.py:116-123:
        sizes (15,30,45,60) on T=60): size_a = (a+1)*T/A.  The one rule for decoding (BaseModel.anchor_sizes) and for
        training from spans."""
        a = self.dpn_head.num_windows
        cfg_sizes = self._anchor_sizes_cfg
        if isinstance(cfg_sizes, (list, tuple)) and len(cfg_sizes) == a:
            return [float(v) for v in cfg_sizes]
        return [(i + 1) * float(num_frames) / a for i in range(a)]

    # packed device weights -------------------------------------------------
    def _head_weights(self, dev):
        def build(ts):
            rw, rb, dw, db = ts
            return (torch.cat([rw[:, :, 0], dw[:, :, 0]], dim=0).contiguous(),
                    torch.cat([rb, db]).contiguous())
        return self._cache.get("heads", self.dpn_head.head_params(), dev, build)

    def _conv_dense(self, dev):
        c = self.dpn_head.conv
        return self._cache.get("conv_dense", (c.weight, c.bias), dev,
                               lambda ts: (ops.pack_conv3(ts[0]), ts[1]))

    def _conv_split(self, dev, winograd=False):
        """Packed weights of the factorised pair form (subject / object halves stacked along M): Winograd
        F(6,3) fragment-major weights (needs D % 32 == 0) or the three direct taps."""
        c = self.dpn_head.conv
        half = self.dpn_head.in_channels // 2
        if winograd:
            return self._cache.get("conv_split_wino63", (c.weight, c.bias), dev,
                                   lambda ts: (ops.pack_conv3_wino63(ts[0], split=half), ts[1]))
        return self._cache.get("conv_split", (c.weight, c.bias), dev,
                               lambda ts: (ops.pack_conv3(ts[0], split=half), ts[1]))

    def _conv_f16x3(self, dev):
        """Split-fp16 F(6,3) weights of the factorised pair form (pack_conv3_wino63_f16x3), for the calls the accuracy
        guard has promoted (BaseModel._winograd).  Its cache key does not start with "conv_split": those are the fp32
        packings."""
        c = self.dpn_head.conv
        half = self.dpn_head.in_channels // 2
        return self._cache.get("wino63_f16x3", (c.weight, c.bias), dev,
                               lambda ts: (ops.pack_conv3_wino63_f16x3(ts[0], split=half), ts[1]))

    def _conv_packed(self, dev, algo):
        """(packed conv weights, bias) for the algorithm BaseModel._conv_algo chose: "f16x3", "wino63" or "direct"."""
        if algo == "f16x3":
            return self._conv_f16x3(dev)
        return self._conv_split(dev, winograd=algo == "wino63")

    def _conv_raw(self, dev):
        """conv.weight as it is (fp32, contiguous, on `dev`): what the accuracy guard recomputes outputs from."""
        return self._cache.get("conv_raw", (self.dpn_head.conv.weight,), dev, lambda ts: ts[0])

    def _bf16_weights(self, dev):
        """bf16 operand set of the factorised path (csrc/tspn_bf16.hip): packed conv / head weights
        in bf16, biases as fp32 tensors holding bf16-rounded values."""
        c = self.dpn_head.conv
        half = self.dpn_head.in_channels // 2
        rnd = lambda t: ops.cast_bf16(t.contiguous()).float()

        def build(ts):
            cw, cb, rw, rb, dw, db = ts
            hw = torch.cat([rw[:, :, 0], dw[:, :, 0]], dim=0).contiguous()
            return (ops.pack_conv3_bf16(cw, split=half), rnd(cb), ops.pack_heads_bf16(hw),
                    rnd(torch.cat([rb, db])))
        return self._cache.get("bf16", (c.weight, c.bias) + tuple(self.dpn_head.head_params()), dev, build)

    def _wrap(self, heads, geom=None):
        a = self.dpn_head.num_windows
        return TemporalProposals(heads[:, :a], heads[:, a:], heads, geom)

    def forward_dense(self, feats):
        """feats: list of materialised [P,C,T] pair tensors (the layout DPNHead consumes)."""
        out = []
        for f in feats:
            dev = _compute_device(f, self.dpn_head.conv.weight)
            packed, cbias = self._conv_dense(dev)
            hw, hb = self._head_weights(dev)
            out.append(self._wrap(ops.temporal_encoder_heads(_f32(f, dev), packed, cbias, hw, hb)))
        return out

    def _train_heads(self, plist):
        """Heads [P,3A,T] of one segment with autograd onto the DPNHead parameters."""
        h = self.dpn_head
        if not h.conv.weight.is_cuda:
            raise RuntimeError("training needs the model on the HIP device (model.cuda())")
        dev = h.conv.weight.device
        rw, rb, dw, db = h.head_params()
        head_w = torch.cat([rw[:, :, 0], dw[:, :, 0]], dim=0)
        head_b = torch.cat([rb, db])
        if plist.has_field("tracklet_feats"):
            f = _f32(plist.get_field("tracklet_feats"), dev)
            if 2 * f.shape[2] != h.in_channels:
                raise ValueError(f"tracklet_feats dim D={f.shape[2]} needs RELPN.DPN.IN_CHANNELS = 2*D")
            return _TemporalHeadsTrackletFn.apply(f, _segment_pairs(plist, f.shape[0], dev), h.conv.weight,
                                                  h.conv.bias, head_w, head_b)
        x = plist.features
        if x.dim() != 3:
            raise ValueError("RELPN.USE_DPN=True needs temporal inputs: PairList.features [P,C,T] or the "
                             "field 'tracklet_feats' [N,T,D] (the reference raises NameError here, "
                             "relpn/dpn.py:24-28)")
        return _TemporalHeadsDenseFn.apply(_f32(x, dev), h.conv.weight, h.conv.bias, head_w, head_b)

    def _forward_train(self, pair_list, target_list):
        """The reference's intent (relpn/dpn.py:40-49; its own code raises NameError):
        duration_proposals = dpn_head(pair feats); loss_duration = BCEWithLogits(duration_proposals,
        target.get_field('duration')), summed over the segments like loss_rel (model.py:62-64).  A target
        field 'relness' [P,A,T], when present, adds `loss_relationness` on the relationness head (loss name
        from relpn/dpn_anchor.py:62-65).  Targets with a field 'spans' instead take _forward_train_spans."""
        if target_list is None:
            raise ValueError("DPN training needs target_list with a 'duration' field [P,2A,T] or a 'spans' field [P,G,2]")
        with_spans = [tlist.has_field("spans") for tlist in target_list]
        if any(with_spans):
            if not all(with_spans) or any(tlist.has_field("duration") for tlist in target_list):
                raise ValueError("DPN training takes either 'spans' [P,G,2] (anchor targets and losses, DESIGN.md §2) or "
                                 "'duration' [P,2A,T] (+ 'relness') in every target of a batch, not both")
            return self._forward_train_spans(pair_list, target_list)
        props, loss_dur, loss_rel = [], 0, None
        for plist, tlist in zip(pair_list, target_list):
            tp = self._wrap(self._train_heads(plist))
            gt = tlist.get_field("duration")
            gt = (gt if isinstance(gt, torch.Tensor) else torch.as_tensor(np.asarray(gt))).to(tp.duration)
            if gt.shape != tp.duration.shape:
                raise ValueError(f"target field 'duration' must be [P,2A,T] = {tuple(tp.duration.shape)}, "
                                 f"got {tuple(gt.shape)}")
            loss_dur = loss_dur + F.binary_cross_entropy_with_logits(tp.duration, gt)
            if tlist.has_field("relness"):
                gr = tlist.get_field("relness")
                gr = (gr if isinstance(gr, torch.Tensor) else torch.as_tensor(np.asarray(gr))).to(tp.relness)
                loss_rel = (0 if loss_rel is None else loss_rel) + F.binary_cross_entropy_with_logits(tp.relness, gr)
            props.append(tp)
        losses = {"loss_duration": loss_dur}
        if loss_rel is not None:
            losses["loss_relationness"] = loss_rel
        return props, losses

    def _forward_train_spans(self, pair_list, target_list):
        """Targets with a field 'spans' int64 [P,G,2] (ground-truth frames [start, end) per pair, end <= start =
        padding): the RPN scheme in one dimension the reference intends (relpn/dpn_anchor.py:50-70) -- anchors labelled by
        IoU, `loss_relationness` on the labelled anchors, `loss_duration_proposal` on the positive ones, on the
        parametrisation decode_spans decodes; both summed over the segments like loss_rel.  With
        RELPN.DPN.SPAN_LOSS.BATCH_SIZE_PER_SEGMENT > 0 the losses of a segment take the balanced mini-batch of
        ops.span_anchor_sample instead of every labelled anchor."""
        props, loss_rel, loss_reg = [], 0, 0
        for plist, tlist in zip(pair_list, target_list):
            heads = self._train_heads(plist)
            gt = tlist.get_field("spans")
            gt = (gt if isinstance(gt, torch.Tensor) else torch.as_tensor(np.asarray(gt))).to(heads.device, torch.int64)
            if gt.dim() != 3 or gt.shape[0] != heads.shape[0] or gt.shape[2] != 2:
                raise ValueError(f"target field 'spans' must be [P,G,2] with P = {heads.shape[0]}, got {tuple(gt.shape)}")
            l_rel, l_reg = _SpanLossFn.apply(heads, gt.contiguous(), self.anchor_sizes(heads.shape[2]), self.span_pos_iou,
                                             self.span_neg_iou, self.span_beta, self._next_span_sample())
            loss_rel, loss_reg = loss_rel + l_rel, loss_reg + l_reg
            props.append(self._wrap(heads))
        return props, {"loss_relationness": loss_rel, "loss_duration_proposal": loss_reg}

    def forward(self, pair_list, target_list=None):
        if self.training:
            return self._forward_train(pair_list, target_list)
        return self.forward_dense([plist.features for plist in pair_list]), {}


class RelPN(nn.Module):
    """PPN + DPN dispatcher (reference lib/modeling/relpn/relpn.py:9-60)."""

    def __init__(self, cfg):
        super().__init__()
        self.use_ppn = cfg.RELPN.USE_PPN
        self.use_dpn = cfg.RELPN.USE_DPN
        self.pair_proposal_network = PPN(cfg)
        self.duration_proposal_network = DPN(cfg, in_channels=cfg.RELPN.DPN.IN_CHANNELS,
                                             num_windows=cfg.RELPN.DPN.NUM_ANCHORS_PER_LOCATION)

    def forward(self, pair_list, target_list=None):
        losses, pair_props, dur_props = {}, None, None
        if self.use_ppn:
            pair_props, l = self.pair_proposal_network(pair_list, target_list)
            losses.update(l)
        if self.use_dpn:
            dur_props, l = self.duration_proposal_network(pair_list, target_list)
            losses.update(l)
        return pair_props, dur_props, losses


def make_relpn(cfg):
    return RelPN(cfg)


def _usable_cpus():
    """Cores this process may really use: the affinity mask capped by the cgroup CPU quota (a container that shows 256
    cores and grants 16 throttles a 128-thread copy to a crawl)."""
    import os
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period) + 0.5)))
    except (OSError, ValueError):
        pass
    return n


_STAGE_POOL = None


def _stage_pool():
    """A few single-threaded copy workers for the pageable -> pinned staging copies (torch's intra-op pool is sized by
    the visible cores, not by the quota, and is shared with everything else the caller runs)."""
    global _STAGE_POOL
    if _STAGE_POOL is None:
        from concurrent.futures import ThreadPoolExecutor
        nt = max(1, min(8, _usable_cpus() - 1))
        _STAGE_POOL = (ThreadPoolExecutor(nt, thread_name_prefix="tspn-stage", initializer=lambda: torch.set_num_threads(1)), nt)
    return _STAGE_POOL


class _HostPipeline:
    """Transfers of one forward whose tracklet features live in HOST memory (what the reference's predict.py:50-57
    hands over: CPU PairLists from a DataLoader): the videos of a group go to the device in chunks on a copy stream,
    the fused pass runs chunk by chunk behind the chunks' copy events, and every chunk's results come back on a third
    stream into pinned tensors - so chunk k+1 uploads, and chunk k-1 downloads, under the encoder of chunk k.
    Pinned sources (`PairList.pin_memory()`, `DataLoader(pin_memory=True)`) are DMA'd as they are; pageable ones
    are staged through a pinned buffer kept here (a multi-threaded host copy), one chunk ahead of the GPU."""

    def __init__(self, dev):
        self.dev = dev
        self.h2d = torch.cuda.Stream(device=dev)
        self.d2h = torch.cuda.Stream(device=dev)
        self.dev_buf, self.pin_buf = {}, {}
        self.compute_done = None        # event on the caller's stream: the last pass that read dev_buf
        self.h2d_done = None            # event on the copy stream: the last DMA out of pin_buf

    @staticmethod
    def schedule(nm, chunk):
        """[(lo, hi)) video ranges.  Only the first upload is exposed, and a fused pass over few videos is less efficient
        than one over many (cfg2: 2.41 ms per video at 2 videos, 2.07 at 4, 1.72 at 16): start with half a chunk, then
        `chunk`, then double while every upload still hides under the pass before it; the last range takes the rest
        (16 videos, chunk 4: 2 + 4 + 10)."""
        chunk = max(1, int(chunk))
        out, lo, size = [], 0, max(1, chunk // 2)
        while lo < nm:
            rest = nm - lo
            nxt = chunk if not out else 2 * size
            hi = nm if (out and rest <= nxt + nxt // 4) else min(nm, lo + size)
            out.append((lo, hi))
            lo, size = hi, nxt
        return out

    def begin(self, src, dtype):
        """Device buffer [nm*n, t, d] for the group + the staging state; nothing is copied yet."""
        nm, (n, t, d) = len(src), tuple(src[0].shape)
        key = (nm, n, t, d, dtype)
        for cache in (self.dev_buf, self.pin_buf):
            if key not in cache and len(cache) >= 4:
                cache.clear()
        if key not in self.dev_buf:
            self.dev_buf[key] = torch.empty((nm * n, t, d), dtype=dtype, device=self.dev)
        self.src, self.n, self.dst = src, n, self.dev_buf[key]
        self.direct = all(x.dtype == dtype and x.is_contiguous() and x.is_pinned() for x in src)
        self.pin = None
        if not self.direct:
            if key not in self.pin_buf:
                self.pin_buf[key] = torch.empty((nm * n, t, d), dtype=dtype, pin_memory=True)
            self.pin = self.pin_buf[key]
            if self.h2d_done is not None:
                self.h2d_done.synchronize()        # the previous forward's DMAs out of the staging buffer are done
        if self.compute_done is not None:
            self.h2d.wait_event(self.compute_done)  # ... and its passes no longer read the device buffer
        # dev_buf comes out of the CALLER stream's pool: a freshly handed-out block may still be in use by kernels
        # queued on that stream (the allocator only orders reuse within one stream), and the first write into it is a
        # DMA on h2d -- so the copy stream starts behind everything the caller has queued so far
        self.h2d.wait_stream(torch.cuda.current_stream(self.dev))
        return self.dst

    def stage(self, lo, hi):
        """Videos [lo, hi): (host copy into the pinned staging buffer,) async DMA on the copy stream; returns the event
        the compute stream has to wait for."""
        n = self.n
        if not self.direct:
            # host copies into the pinned staging buffer (cast included), row blocks spread over the copy workers
            pool, nt = _stage_pool()
            parts = max(1, min(n, -(-nt // (hi - lo))))
            step = -(-n // parts)
            jobs = [(v * n + r, min(v * n + r + step, (v + 1) * n), v, r) for v in range(lo, hi) for r in range(0, n, step)]
            list(pool.map(lambda j: self.pin[j[0]:j[1]].copy_(self.src[j[2]][j[3]:j[3] + (j[1] - j[0])]), jobs))
        for v in range(lo, hi):
            x = self.src[v] if self.direct else self.pin[v * n:(v + 1) * n]
            with torch.cuda.stream(self.h2d):
                self.dst[v * n:(v + 1) * n].copy_(x, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(self.h2d)
        if not self.direct:
            self.h2d_done = ev
        return ev

    def download(self, main, pairs):
        """`pairs` = [(pinned host tensor, device tensor), ...] of one chunk, complete on `main` now: copied back on the
        download stream."""
        ev = torch.cuda.Event()
        ev.record(main)
        self.d2h.wait_event(ev)
        with torch.cuda.stream(self.d2h):
            for host, devt in pairs:
                host.copy_(devt, non_blocking=True)

    def finish(self, main):
        ev = torch.cuda.Event()
        ev.record(main)
        self.compute_done = ev
        self.d2h.synchronize()             # the caller gets host tensors: they must be complete


class _ScorerF32:
    """How BaseModel scores one group of fp32 segments on `dev`: the weight set out of the model's caches, the shape
    figures callers size outputs by (`dtype`, `rows` = 3A, `K`), and the one call of each fused and span entry.
    _ScorerBf16 has the same methods; callers pick one of the two by the features' dtype (_scorer_kind) and know nothing
    else about the operand type.

    The fused pass's weights are resolved on first use (`rows`, `workspace_bytes`, `run`), never by the span methods:
    choosing the conv algorithm (BaseModel._conv_algo) reads and clears the device's guard words, counts clean reads and
    may promote or fall back, so it happens once per fp32 group and forward, in group order, behind the host-pipeline
    test and behind the pair table of a resident group."""
    dtype = torch.float32

    def __init__(self, model, dev, d):
        self.model, self.dev, self.d = model, dev, d
        cls = model.classifier.rel_predictor
        self.K = cls.weight.shape[0]
        self.cw, self.cb = model.classifier._cache.get("cls", (cls.weight, cls.bias), dev, lambda ts: ts)

    @functools.cached_property
    def _fused(self):
        """(packed conv, conv bias, head weight, head bias, raw conv weight and rows of the guard's spot check or
        (None, 0), conv_algo of the workspace query)."""
        m, dpn = self.model, self.model.relpn.duration_proposal_network
        hw, hb = dpn._head_weights(self.dev)
        # temporal conv algorithm: RELPN.DPN.CONV_ALGO = "auto" (Winograd F(6,3) when D % 32 == 0: 4/9 of the
        # MFMA work; its fp32 error bound is in DESIGN.md §4) or "direct" (the k=3 taps as one implicit GEMM)
        algo = m._conv_algo(self.d, self.dev)
        packed, cbias = dpn._conv_packed(self.dev, algo)
        craw, crows = (dpn._conv_raw(self.dev), m.conv_check_rows) if algo != "direct" and m.conv_check_rows > 0 else (None, 0)
        return packed, cbias, hw, hb, craw, crows, _abi.CONV_WINOGRAD63_F16X3 if algo == "f16x3" else 0

    @property
    def rows(self):
        return self._fused[3].numel()

    def workspace_bytes(self, nm, n, t, d, P, canonical):
        return ops.fused_workspace_bytes(nm, n, t, d, self.rows // 3, self.K, P, conv_algo=self._fused[6])

    def run(self, feats, pairs, nm, n, workspace, canonical, conv_events, logits_event, out_heads=None, out_logits=None):
        packed, cbias, hw, hb, craw, crows, _ = self._fused
        return ops.forward_fused(feats, pairs, nm, n, packed, cbias, hw, hb, self.cw, self.cb, workspace=workspace,
                                 check_pairs=False, canonical_pairs=canonical, conv_events=conv_events,
                                 conv_weight=craw, conv_check=crows, logits_event=logits_event,
                                 out_heads=out_heads, out_logits=out_logits)

    def span_logits(self, feats, pairs, spans):
        """RelOIPool over each pair's span + predicate head: sigmoid logits [P,K]."""
        return ops.span_predicate(feats, pairs, spans, self.cw, self.cb)

    def span_relations(self, feats, pairs, sp, clog, topk_per_span, topk_per_seg):
        return ops.decode_span_relations(feats, pairs, sp["span"], sp["score"], sp["count"], self.cw, self.cb, clog,
                                         topk_per_span=topk_per_span, topk_per_seg=topk_per_seg, check_pairs=False)


class _ScorerBf16:
    """_ScorerF32 for bf16 'tracklet_feats': the bf16-operand kernels (BASELINE config 3) and their semantics
    (DESIGN.md §2); a group with an explicit pair table goes through the pair-list stage.  No conv algorithm to choose;
    the packed weights are still made on first use, where the fused sites have always made them."""
    dtype = torch.bfloat16

    def __init__(self, model, dev, d):
        if d % 16:
            raise ValueError(f"the bf16 path needs D % 16 == 0 (D={d})")
        self.model, self.dev = model, dev
        self.K = model.classifier.rel_predictor.weight.shape[0]

    @functools.cached_property
    def _fused(self):
        return self.model.relpn.duration_proposal_network._bf16_weights(self.dev) + self.model._cls_bf16(self.dev)

    @property
    def rows(self):
        return self._fused[3].numel()

    def workspace_bytes(self, nm, n, t, d, P, canonical):
        return ops.fused_bf16_workspace_bytes(nm, n, t, d, self.rows // 3, self.K, P, canonical_pairs=canonical)

    def run(self, feats, pairs, nm, n, workspace, canonical, conv_events, logits_event, out_heads=None, out_logits=None):
        return ops.forward_fused_bf16(feats, pairs, nm, n, *self._fused, workspace=workspace, conv_events=conv_events,
                                      logits_event=logits_event, out_heads=out_heads, out_logits=out_logits,
                                      canonical_pairs=canonical, check_pairs=False)

    def span_logits(self, feats, pairs, spans):
        return ops.span_predicate_bf16(feats, pairs, spans, *self.model._span_cls_bf16(self.dev), self.K)

    def span_relations(self, feats, pairs, sp, clog, topk_per_span, topk_per_seg):
        return ops.decode_span_relations_bf16(feats, pairs, sp["span"], sp["score"], sp["count"],
                                              *self.model._span_cls_bf16(self.dev), self.K, clog,
                                              topk_per_span=topk_per_span, topk_per_seg=topk_per_seg, check_pairs=False)


def _scorer_kind(feats):
    """The scorer class of a segment's 'tracklet_feats': bf16 features select the bf16 operand set, anything else fp32."""
    return _ScorerBf16 if isinstance(feats, torch.Tensor) and feats.dtype == torch.bfloat16 else _ScorerF32


_LogitsToken = namedtuple("_LogitsToken", ["device", "logits", "stream", "host_ids"], defaults=[None])
_LogitsToken.__doc__ = """The last single-group fused pass, for `decode`: device index, its batched logits tensor (kept
alive here: its address cannot be handed to another tensor while the token stands), the caller's stream, and `host_ids` =
(data_ptr, version) of the host tensors handed out for them, or None when the pass returned views of `logits` itself."""


class BaseModel(_CachedWeightsMixin, nn.Module):
    """RelPN -> RelOIPool -> predicate classifier (reference lib/modeling/model.py:7-65)."""

    def __init__(self, cfg):
        super().__init__()
        self.use_ppn = cfg.RELPN.USE_PPN
        self.use_dpn = cfg.RELPN.USE_DPN
        self.relpn = make_relpn(cfg)
        self.rel_of_interest_pool = RelOIPool()
        self.classifier = RelationPredictor(in_channels=cfg.PREDICT.FEATURE_DIM,
                                            out_channels=cfg.PREDICT.PREDICATE_NUM,
                                            fuse_preprocess=getattr(cfg.PREDICT, "FUSE_PREPROCESS", False))
        self.pool_top_span = bool(getattr(cfg.RELPN.DPN, "POOL_TOP_SPAN", False))
        # build extension: train the predicate head of tracklet samples on ground-truth-span-pooled rows
        self.pool_gt_span = bool(getattr(cfg.RELPN.DPN, "POOL_GT_SPAN", False))
        # build extension: also return the bbox half of the pair builder (relative geometry [P,8,T]) from the
        # eval forward.  Nothing downstream of forward consumes it, so it is off unless asked for
        # (`model.pair_geometry(pair_list)` computes it on demand).
        self.pair_geometry_in_forward = bool(getattr(cfg.RELPN.DPN, "PAIR_GEOMETRY", False))
        self._workspaces = {}        # (device index, stream) -> uint8 workspace of the fused pass, grown on demand
        self._pair_tables = {}       # (device, B, N) -> (batched canonical pair table [B*P,2], per-video table [B,P,2])
        self._conv_events = None     # optional (begin, end) torch.cuda.Event pair around the dominant kernel
        # build extension: the small latency-bound kernels of a step (PPN; the top-k triplet decode of `decode`) run on
        # a second HIP stream under the encoder of the same forward: PPN needs the class logits only, decode only the
        # predicate logits, which the fused pass computes FIRST and signals with an event.  Both join the caller's
        # stream before their results are handed out, so the caller sees ordinary stream semantics.
        self.overlap_tail = bool(getattr(cfg.RELPN, "OVERLAP_TAIL", True))
        self._side = {}              # device index -> (side stream, logits-ready event)
        self._logits_token = None    # _LogitsToken of the last fused pass that had a single group
        # host-resident inputs (predict.py hands CPU PairLists): videos per pipelined chunk, see _HostPipeline
        self.host_chunk_videos = int(getattr(cfg.RELPN.DPN, "HOST_CHUNK_VIDEOS", 4))
        self._host_pipes = {}
        self.conv_algo = str(getattr(cfg.RELPN.DPN, "CONV_ALGO", "auto"))
        if self.conv_algo not in ("auto", "direct"):
            raise ValueError(f"RELPN.DPN.CONV_ALGO must be auto or direct (got {self.conv_algo})")
        # accuracy guard of "auto" (round 6): every fused pass that runs F(6,3) also spot-checks CONV_CHECK_ROWS output
        # rows against a float64 recomputation (csrc/tspn_conv_guard.hip); a measured error above CONV_TOL makes this
        # model warn once and use the direct kernel from its next call on (`conv_fallback`)
        self.conv_tol = float(getattr(cfg.RELPN.DPN, "CONV_TOL", 1e-4))
        self.conv_check_rows = int(getattr(cfg.RELPN.DPN, "CONV_CHECK_ROWS", 128))
        self.conv_fallback = False
        self.conv_err_seen = 0.0     # largest spot-check error this model has read back so far
        # split-fp16 F(6,3) (TSPN_CONV_WINOGRAD63_F16X3): once CONV_F16X3_AFTER calls have read a guard measurement
        # <= CONV_TOL from the fp32 F(6,3) calls before them, and the shape passes the split kernels' gate, the calls
        # from then on run the split form (spot-checked the same way); CONV_F16X3 = False keeps the fp32 form
        self.conv_f16x3 = bool(getattr(cfg.RELPN.DPN, "CONV_F16X3", True))
        self.conv_f16x3_after = max(1, int(getattr(cfg.RELPN.DPN, "CONV_F16X3_AFTER", 4)))
        self.conv_clean_reads = 0    # calls that found a standing clean measurement of the fp32 form
        self.conv_promoted = False

    def forward(self, pair_list, target_list=None):
        if self.training:
            return self._forward_train(pair_list, target_list)
        return self._forward_test(pair_list)

    _conv_guard_owner = {}       # device index -> weakref of the model whose guarded F(6,3) pass ran last on that device

    def _winograd(self, d, dev):
        """Temporal conv algorithm of this call: True = Winograd F(6,3) (RELPN.DPN.CONV_ALGO "auto", D % 32 == 0, and the
        accuracy guard has not tripped).  Reads what the guard measured in EARLIER calls from the device's status block
        (pinned host memory: no synchronisation) -- the contract is a plain fp32 Conv1d (reference relpn/dpn.py:69-73) to
        1e-4, and F(6,3)'s fp32 error depends on the data."""
        if self.conv_algo != "auto" or d % 32 or self.conv_fallback:
            return False
        if self.conv_check_rows > 0:
            words = ops.status_words(dev)
            # the words are per DEVICE: a measurement belongs to the model whose guarded pass ran last there; what another
            # model (or a direct caller of ops.conv3_spot_check) left is discarded, not attributed to this one
            owner = BaseModel._conv_guard_owner.get(dev.index)
            mine = owner is not None and owner() is self
            BaseModel._conv_guard_owner[dev.index] = weakref.ref(self)
            if not mine:
                words[_abi.STATUS_CONV_ERR] = 0
                words[_abi.STATUS_CONV_CHECKS] = 0
                return True
            err = float(words[_abi.STATUS_CONV_ERR:_abi.STATUS_CONV_ERR + 1].view(np.float32)[0])
            self.conv_err_seen = max(self.conv_err_seen, err)
            if err <= self.conv_tol and int(words[_abi.STATUS_CONV_CHECKS]) > 0 and self.conv_f16x3 and d % 128 == 0:
                # one more call that finds the fp32 passes before it measured within CONV_TOL; the split form waits for
                # CONV_F16X3_AFTER of them (a pass's spot check samples one batch: several batches before the switch)
                self.conv_clean_reads += 1
                self.conv_promoted = self.conv_clean_reads >= self.conv_f16x3_after
            if not (err <= self.conv_tol):     # a non-finite measurement (+Inf: a NaN / Inf where float64 has none) trips
                checks = int(words[_abi.STATUS_CONV_CHECKS])
                words[_abi.STATUS_CONV_ERR] = 0
                words[_abi.STATUS_CONV_CHECKS] = 0
                self.conv_fallback = True
                warnings.warn(
                    f"TSPN: the Winograd F(6,3) temporal conv measured an absolute error of {err:.3g} against float64 "
                    f"on this model's inputs ({checks} outputs spot-checked), above RELPN.DPN.CONV_TOL = {self.conv_tol:g}"
                    + (" (inf: a NaN or Inf output where float64 has a different value -- non-finite inputs, which F(6,3) "
                       "smears over their sextet)" if not np.isfinite(err) else "") + ": "
                    "using the direct kernel (reference-order fp32 taps, about 2.2x slower) from this call on.  Set "
                    "RELPN.DPN.CONV_ALGO = 'direct' to start there, or raise CONV_TOL if the features' scale makes "
                    "1e-4 absolute meaningless (INTEGRATION.md §3).", RuntimeWarning, stacklevel=3)
                return False
        return True

    def _conv_algo(self, d, dev):
        """"f16x3", "wino63" or "direct" for this call (see _winograd; the split form needs D % 128 == 0 here, which
        keeps the small-D models on the fp32 form)."""
        if not self._winograd(d, dev):
            return "direct"
        return "f16x3" if self.conv_promoted else "wino63"

    # ------------------------------------------------------------------ train
    def _forward_train(self, pair_list, target_list):
        loss_dict = {}
        duration_proposals = None
        feats = [plist.features for plist in pair_list]
        targets = [tlist.target for tlist in target_list]
        if self.use_ppn or self.use_dpn:
            _, duration_proposals, relpn_losses = self.relpn(pair_list, target_list)
            loss_dict.update(relpn_losses)
        if duration_proposals is not None:
            # RelOIPool over the segment; tracklet samples: cat of the two tracklet means
            dev = self.classifier.rel_predictor.weight.device
            feats = [self._pooled_pair_feats(p, dev) if self._is_tracklet_sample(p) else _f32(p.features, dev)
                     for p in pair_list]
        reloi_feats = self.rel_of_interest_pool(feats, duration_proposals)
        # RELPN.DPN.POOL_GT_SPAN: tracklet samples train the head on ground-truth-span-pooled rows;
        # samples in the [P,F] baseline form keep the rows they bring
        spanned = {i for i, p in enumerate(pair_list) if self.pool_gt_span and self._is_tracklet_sample(p)}
        loss_relation = self._span_pooled_loss_rel(pair_list, target_list, sorted(spanned)) if spanned else 0
        for i, (reloi_feat, target) in enumerate(zip(reloi_feats, targets)):
            if i in spanned:
                continue
            rel_logit = self.classifier(reloi_feat)
            loss_relation = loss_relation + F.binary_cross_entropy(rel_logit, target)
        loss_dict["loss_rel"] = loss_relation
        return loss_dict

    SPAN_TARGET_FIELDS = (("spans", torch.int64), ("span_count", torch.int32), ("span_labels", torch.float32))

    def _span_pooled_loss_rel(self, pair_list, target_list, members):
        """loss_rel of the tracklet samples `members` under RELPN.DPN.POOL_GT_SPAN: per group of equal-shape segments one
        _SpanPredicateLossFn call over the group's tracklets back to back, its pair tables with global ids and the
        target fields 'spans' [P,G,2], 'span_count' [P] and 'span_labels' [P,G,K] of its segments; the sum over the
        segments, like every loss_rel."""
        w, b = self.classifier.rel_predictor.weight, self.classifier.rel_predictor.bias
        if not w.is_cuda:
            raise RuntimeError("training needs the model on the HIP device (model.cuda())")
        dev, groups = w.device, {}
        for i in members:
            f = _f32(pair_list[i].get_field("tracklet_feats"), dev)
            if f.dim() != 3:
                raise ValueError(f"tracklet_feats must be [N,T,D], got {tuple(f.shape)}")
            groups.setdefault(tuple(f.shape), []).append((i, f))
        loss = 0
        for (n, _, _), group in groups.items():
            feats = _consecutive_view([f for _, f in group])
            if feats is None:
                feats = torch.cat([f for _, f in group])
            pairs, offsets, fields = [], [0], {name: [] for name, _ in self.SPAN_TARGET_FIELDS}
            for k, (i, _) in enumerate(group):
                p = _segment_pairs(pair_list[i], n, dev)
                for name, dtype in self.SPAN_TARGET_FIELDS:
                    if not target_list[i].has_field(name):
                        raise ValueError(f"RELPN.DPN.POOL_GT_SPAN needs the target field '{name}' (dataset.proposal_pair_list "
                                         "with gt_rel_insts, max_spans and span_labels=True)")
                    v = target_list[i].get_field(name)
                    if not isinstance(v, torch.Tensor) or v.dtype != dtype or v.shape[0] != p.shape[0]:
                        raise ValueError(f"target field '{name}' must be a {dtype} tensor with P = {p.shape[0]} rows")
                    fields[name].append(v.to(dev))
                pairs.append(p + k * n)
                offsets.append(offsets[-1] + p.shape[0])
            one = len(group) == 1
            cat = lambda ts: ts[0].contiguous() if one else torch.cat(ts)   # noqa: E731
            pair_off = None if one else torch.tensor(offsets, dtype=torch.int64, device=dev)
            loss = loss + _SpanPredicateLossFn.apply(feats.contiguous(), cat(pairs), cat(fields["spans"]),
                                                     cat(fields["span_count"]), cat(fields["span_labels"]),
                                                     w.contiguous(), b.contiguous(), pair_off)
        return loss

    # ------------------------------------------------------------------- eval
    @staticmethod
    def _is_tracklet_sample(plist):
        return plist.has_field("tracklet_feats")

    @staticmethod
    def _pooled_pair_feats(plist, dev):
        """[P, 2D] = cat(mean_t f[s], mean_t f[o]): the segment-pooled pair feature of a tracklet sample."""
        f = _f32(plist.get_field("tracklet_feats"), dev)
        return ops.pair_rows(ops.temporal_mean(f, layout_tc=True), _segment_pairs(plist, f.shape[0], dev))

    def profile_conv_events(self, events):
        """(begin, end) torch.cuda.Event pair (enable_timing=True, recorded once) re-recorded around the dominant
        kernel of the next fused forwards — the hook bench.py's roofline figure uses; None switches it off."""
        self._conv_events = events

    def _workspace(self, dev, nbytes):
        """Scratch of the fused pass, kept on the module and reused by every forward on the same (device, stream):
        launches on one stream are ordered, so the buffer is free again when the next pass starts."""
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        ws = self._workspaces.get(key)
        if ws is None or ws.numel() < nbytes:
            self._workspaces.pop(key, None)
            while len(self._workspaces) >= 4:        # streams come and go: never hold more than four (5 GB each at cfg2)
                self._workspaces.pop(next(iter(self._workspaces)))
            ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)
            self._workspaces[key] = ws
        return ws

    def _canonical_pairs(self, dev, b, n):
        """(global pair table [B*N(N-1), 2] with video b's ids offset by b*N, per-video table [B, N(N-1), 2]) of B
        equal-N videos, built once per (device, B, N)."""
        key = (str(dev), b, n)
        hit = self._pair_tables.get(key)
        if hit is None:
            if len(self._pair_tables) >= 16:
                self._pair_tables.clear()
            local = ops.pair_index(n, dev)
            allp = (local.unsqueeze(0) + (torch.arange(b, device=dev, dtype=torch.int64) * n).view(b, 1, 1))
            hit = (allp.reshape(-1, 2).contiguous(), local.unsqueeze(0).expand(b, -1, -1).contiguous())
            self._pair_tables[key] = hit
        return hit

    def _group_pair_table(self, customs, dev, n):
        """Pair table of one group of equal-shape segments for a fused pass (either operand type): `customs` holds, per
        member, its validated-here 'tracklet_pairs' as a host int64 [P,2] of local ids, or None for all ordered pairs.
        Returns (global table [sum P, 2] on `dev` with member k's ids offset by k*n, rows per member, whether it is the
        canonical table of every member)."""
        nm = len(customs)
        if all(p is None for p in customs):
            allp, _ = self._canonical_pairs(dev, nm, n)
            return allp, [n * (n - 1)] * nm, True
        pairs = []
        for k, p in enumerate(customs):
            if p is None:
                pairs.append(ops.pair_index(n, dev, base=k * n))
                continue
            if p.dim() != 2 or p.shape[1] != 2:
                raise ValueError("tracklet_pairs must be [P,2]")
            if p.numel() and (int(p.min()) < 0 or int(p.max()) >= n):
                raise IndexError("tracklet_pairs index out of range")
            pairs.append(p.to(dev) + k * n)
        return torch.cat(pairs).contiguous(), [p.shape[0] for p in pairs], False

    def _side_stream(self, dev):
        hit = self._side.get(dev.index)
        if hit is None:
            ev = torch.cuda.Event()
            with torch.cuda.device(dev):
                side = torch.cuda.Stream(device=dev)
                ev.record()                        # creates the HIP event handle the ABI hook re-records
            hit = (side, ev)
            self._side[dev.index] = hit
        return hit

    def _forward_test(self, pair_list):
        with torch.no_grad():
            if self.use_dpn and len(pair_list) and all(self._is_tracklet_sample(p) for p in pair_list):
                return self._forward_test_fused(pair_list)
            if self.use_dpn and any(p.features.dim() != 3 for p in pair_list):
                raise ValueError(
                    "RELPN.USE_DPN=True needs temporal inputs: either PairList.features of shape "
                    "[P,C,T] or the fields 'tracklet_feats' [N,T,D] (+ 'tracklet_boxes'); got 2-D "
                    "features (the reference raises NameError here, relpn/dpn.py:24-28)")
            feats = [plist.features for plist in pair_list]
            pair_proposals, duration_proposals, _ = self.relpn(pair_list)
            reloi_feats = self.rel_of_interest_pool(
                [_f32(f, _compute_device(f, self.classifier.rel_predictor.weight)) if f.dim() == 3 else f
                 for f in feats], duration_proposals)
            rel_logits = [self.classifier(r).to(f.device) for r, f in zip(reloi_feats, feats)]
            if duration_proposals is not None:
                duration_proposals = [TemporalProposals(*(t.to(f.device) if t is not None else None for t in d))
                                      for d, f in zip(duration_proposals, feats)]
            return pair_proposals, duration_proposals, rel_logits

    def _forward_test_fused(self, pair_list):
        """Temporal path on tracklet tensors: one fused HIP pass per group of equal-shape segments."""
        dpn = self.relpn.duration_proposal_network
        cls = self.classifier.rel_predictor
        first = pair_list[0].get_field("tracklet_feats")
        dev = _compute_device(first, dpn.dpn_head.conv.weight)
        d_feat = first.shape[2]
        if 2 * d_feat != dpn.dpn_head.in_channels:
            raise ValueError(f"tracklet_feats dim D={d_feat} needs RELPN.DPN.IN_CHANNELS = 2*D "
                             f"(got {dpn.dpn_head.in_channels})")
        if cls.in_features != 2 * d_feat:
            raise ValueError(f"PREDICT.FEATURE_DIM must equal 2*D = {2 * d_feat} on the temporal path "
                             f"(got {cls.in_features})")
        main = torch.cuda.current_stream(dev)
        overlap = self.overlap_tail and all(p.get_field("tracklet_feats").is_cuda for p in pair_list)
        side, ev_logits = self._side_stream(dev) if overlap else (None, None)
        customs = [_pairs_field(p) for p in pair_list]
        groups = {}
        for i, plist in enumerate(pair_list):
            f = plist.get_field("tracklet_feats")
            # segments with an explicit pair table are scored on their own
            groups.setdefault((tuple(f.shape), i + 1 if customs[i] is not None else 0, _scorer_kind(f)), []).append(i)
        if side is not None:
            # everything the side stream reads that THIS call may build lazily is built here, on the caller's stream,
            # before the side stream is made to wait for it: the PPN weight copies and the canonical pair tables of
            # every group (read by the pair-geometry launch here and by `decode` later)
            if self.use_ppn:
                self.relpn.pair_proposal_network.device_weights(dev)
            for (shape, custom_key, _), members in groups.items():
                if custom_key == 0:
                    self._canonical_pairs(dev, len(members), shape[0])
            side.wait_stream(main)                 # class logits / boxes may have been produced on the caller's stream
        pair_proposals = None
        if self.use_ppn:
            if overlap and all(p.get_field("track_cls_logits").is_cuda for p in pair_list):
                with torch.cuda.stream(side):
                    pair_proposals, _ = self.relpn.pair_proposal_network(pair_list)
                    for t in pair_proposals:
                        t.record_stream(main)      # allocated under the side stream, consumed on the caller's
            else:
                pair_proposals, _ = self.relpn.pair_proposal_network(pair_list)
        self._logits_token = None
        join_side = False

        n_seg = len(pair_list)
        durations, logits = [None] * n_seg, [None] * n_seg
        track = len(groups) == 1                   # the logits-ready event and the token stand for ONE fused pass
        for (shape, custom_key, kind), members in groups.items():
            n, t, d = shape
            nm = len(members)
            src = [pair_list[i].get_field("tracklet_feats") for i in members]
            scorer = kind(self, dev, d)
            if (self.host_chunk_videos > 0 and custom_key == 0 and not self.pool_top_span and n * (n - 1) > 0
                    and all(isinstance(x, torch.Tensor) and not x.is_cuda for x in src)):
                # host-resident features, canonical pair table: chunked upload / compute / download pipeline
                self._forward_host_group(pair_list, members, shape, scorer, dev, durations, logits, track_token=track)
                continue
            feats = _batch_rows(src, dev, scorer.dtype)
            allp, counts, canonical = self._group_pair_table(
                [None if customs[i] is None else customs[i].cpu() for i in members], dev, n)
            if not canonical and side is not None and self.pair_geometry_in_forward:
                side.wait_stream(main)     # the geometry launch on the side stream reads this table
            need = scorer.workspace_bytes(nm, n, t, d, allp.shape[0], canonical)
            heads, lg = scorer.run(feats, allp, nm, n, self._workspace(dev, need), canonical, self._conv_events,
                                   ev_logits if track else None)
            if self.pool_top_span and allp.shape[0]:
                # RelOIPool over each pair's best span (decode + NMS, top-1) instead of the whole segment, in the
                # group's own semantics: canonical and custom tables alike
                top = ops.decode_spans(heads, self.anchor_sizes(t), top_k=1)["span"][:, 0].contiguous()
                lg = scorer.span_logits(feats, allp, top)
            if overlap and track and not self.pool_top_span:
                # `decode` may start behind the logits-ready event of THIS pass (same logits tensor, same caller stream)
                self._logits_token = _LogitsToken(dev.index, lg, main.cuda_stream)
            geom = None
            if self.pair_geometry_in_forward:
                if side is not None and _have_boxes(pair_list, members, on_device=True):
                    # the bbox half of the pair builder needs the boxes only: second stream, under the encoder
                    with torch.cuda.stream(side):
                        geom = self._pair_geometry_batch(pair_list, members, allp, dev)
                        if geom is not None:
                            geom.record_stream(main)
                    join_side = True
                else:
                    geom = self._pair_geometry_batch(pair_list, members, allp, dev)
            # per-segment results are VIEWS of the batched outputs (copies only when a segment's inputs live on
            # another device, e.g. the host tensors predict.py hands over)
            off = 0
            for k, i in enumerate(members):
                src_dev = src[k].device
                sl = slice(off, off + counts[k])
                durations[i] = dpn._wrap(heads[sl].to(src_dev), None if geom is None else geom[sl].to(src_dev))
                logits[i] = lg[sl].to(src_dev)
                off += counts[k]
        if side is not None and (self.use_ppn or join_side):
            main.wait_stream(side)                 # PPN / geometry are complete for whatever the caller does next
        return pair_proposals, durations, logits

    @staticmethod
    def _host_chunk_schedule(nm, chunk):
        """Video ranges the host-input pipeline scores one after the other (bench.py reads the last one)."""
        return _HostPipeline.schedule(nm, chunk)

    def _forward_host_group(self, pair_list, members, shape, scorer, dev, durations, logits, track_token):
        """One group of equal-shape segments whose `tracklet_feats` are HOST tensors (the reference's predict.py:50-57
        hands CPU PairLists): upload, fused pass and download run as a three-stage pipeline over chunks of videos
        (_HostPipeline); results are pinned host tensors, complete when this returns (same device as the inputs,
        reference model.py:53-65).  Same kernels, same per-video results as the resident path."""
        dpn = self.relpn.duration_proposal_network
        n, t, d = shape
        nm, per = len(members), n * (n - 1)
        src = [pair_list[i].get_field("tracklet_feats") for i in members]
        pipe = self._host_pipes.get(dev.index)
        if pipe is None:
            pipe = self._host_pipes[dev.index] = _HostPipeline(dev)
        main = torch.cuda.current_stream(dev)
        a3, k_out = scorer.rows, scorer.K
        chunks = pipe.schedule(nm, self.host_chunk_videos)
        feats = pipe.begin(src, scorer.dtype)
        heads_dev = torch.empty((nm * per, a3, t), dtype=torch.float32, device=dev)
        lg_dev = torch.empty((nm * per, k_out), dtype=torch.float32, device=dev)
        heads_host = torch.empty((nm * per, a3, t), dtype=torch.float32, pin_memory=True)
        lg_host = torch.empty((nm * per, k_out), dtype=torch.float32, pin_memory=True)
        want_geom = self.pair_geometry_in_forward and _have_boxes(pair_list, members)
        geom_host = torch.empty((nm * per, 8, t), dtype=torch.float32, pin_memory=True) if want_geom else None
        # like heads_dev / lg_dev: lives until finish() has synchronised the download stream (a per-chunk temporary
        # would go back to the caller stream's pool while d2h still reads it)
        geom_dev = torch.empty((nm * per, 8, t), dtype=torch.float32, device=dev) if want_geom else None
        cmax = max(hi - lo for lo, hi in chunks)
        ws = self._workspace(dev, scorer.workspace_bytes(cmax, n, t, d, cmax * per, True))
        # the small side inputs go up NOW, while the caller's stream is empty: a blocking .to(device) issued after a
        # pass has been queued would wait for that pass and stall the pipeline
        boxes_dev = _batch_rows([pair_list[i].get_field("tracklet_boxes") for i in members], dev) if want_geom else None
        ready = pipe.stage(*chunks[0])
        for k, (lo, hi) in enumerate(chunks):
            c = hi - lo
            main.wait_event(ready)
            allp, _ = self._canonical_pairs(dev, c, n)
            rows = slice(lo * per, hi * per)
            scorer.run(feats[lo * n:hi * n], allp, c, n, ws, True, self._conv_events if k == len(chunks) - 1 else None, None,
                       out_heads=heads_dev[rows], out_logits=lg_dev[rows])
            back = [(heads_host[rows], heads_dev[rows]), (lg_host[rows], lg_dev[rows])]
            if want_geom:
                ops.pair_gather(None, boxes_dev[lo * n:hi * n], allp, want_feat=False, check_pairs=False,
                                out_geom=geom_dev[rows])
                back.append((geom_host[rows], geom_dev[rows]))
            pipe.download(main, back)
            if k + 1 < len(chunks):
                ready = pipe.stage(*chunks[k + 1])         # host staging of chunk k+1 runs while the GPU works on chunk k
        pipe.finish(main)
        for k, i in enumerate(members):
            sl = slice(k * per, (k + 1) * per)
            durations[i] = dpn._wrap(heads_host[sl], None if geom_host is None else geom_host[sl])
            logits[i] = lg_host[sl]
        if track_token:
            # `decode` on these very host tensors reads the device copy instead of uploading them again
            self._logits_token = _LogitsToken(dev.index, lg_dev, main.cuda_stream,
                                              tuple((logits[i].data_ptr(), logits[i]._version) for i in members))

    @staticmethod
    def _pair_geometry_batch(pair_list, members, allp, dev):
        """The bbox half of the N^2 pair builder for one group of equal-shape segments, ONE launch: relative
        box geometry [P_total, 8, T] of every scored pair (pair_geometry_kernel: one lane per (pair, frame),
        the motion channels through a wavefront shuffle).  None unless every segment carries 'tracklet_boxes'."""
        if not _have_boxes(pair_list, members) or allp.shape[0] == 0:
            return None
        boxes = _batch_rows([pair_list[i].get_field("tracklet_boxes") for i in members], dev)
        _, geom = ops.pair_gather(None, boxes, allp, want_feat=False, check_pairs=False)   # allp was validated above
        return geom

    def decode(self, pair_list, rel_logits, topk_per_pair=20, topk_per_seg=200, num_obj=35, overlap=True):
        """Top-k triplet decode of `forward`'s rel_logits on the GPU (replaces the Python of
        reference lib/modeling/predict.py:59-117).  Per segment returns
        (scores [M], triplets int64 [M,3] = (subject class, predicate, object class), pair_tids [M,2]).

        Baseline segments (2-D `features` [P,F>=70]) reproduce predict.py:88-89 as is: class =
        argmax of feature row (N-1)*tid, columns 0:35 / 35:70.  Tracklet segments use
        'track_cls_logits' [N,35] directly.  Segments with < 2 tracklets yield empty results
        (predict.py:61-64 skips them).

        Stream contract of the overlapped tail (`RELPN.OVERLAP_TAIL`): when `rel_logits` are the very tensors the last
        `forward` on this stream returned, the decode runs on the module's side stream behind that forward's
        logits-ready event, i.e. under its encoder.  The side stream was ordered after the caller's stream at the START
        of that forward, so `pair_list`'s fields must be the ones that forward was given; class logits (re)written on
        the caller's stream BETWEEN forward and decode are not waited for — pass `overlap=False` (or set
        `model.overlap_tail = False`) for such a decode."""
        out = [None] * len(pair_list)
        groups = {}
        for i, (plist, lg) in enumerate(zip(pair_list, rel_logits)):
            n = int(plist.get_field("num_tracklets")) if plist.has_field("num_tracklets") else None
            quirk = plist.features.dim() == 2 and plist.features.shape[1] >= 2 * num_obj
            if n is None:
                n = int(plist.get_field("track_cls_logits").shape[0])
            if n <= 1 or lg.shape[0] == 0:
                dev = lg.device
                out[i] = (torch.empty(0, device=dev), torch.empty((0, 3), dtype=torch.int64, device=dev),
                          torch.empty((0, 2), dtype=torch.int64, device=dev))
                continue
            groups.setdefault((n, tuple(lg.shape), quirk, tuple(plist.features.shape) if quirk else None), []).append(i)
        for (n, lshape, quirk, _), members in groups.items():
            dev = _compute_device(*[rel_logits[i] for i in members])
            nm = len(members)
            tok = self._logits_token
            if (tok is not None and tok.host_ids is not None and tok.device == dev.index
                    and tok.logits.numel() == nm * lshape[0] * lshape[1]
                    and tok.stream == torch.cuda.current_stream(dev).cuda_stream
                    and tok.host_ids == tuple((rel_logits[i].data_ptr(), rel_logits[i]._version) for i in members)):
                # the host tensors the last forward handed out, untouched: their device copy is still there
                lg = tok.logits.view(nm, lshape[0], lshape[1])
            else:
                lg = _batch_rows([rel_logits[i] for i in members], dev).view(nm, lshape[0], lshape[1])
            # these are the logits of the last fused forward, still on the stream that produced them: decode on the
            # side stream behind their ready-event, i.e. UNDER that forward's encoder, and join afterwards
            main = torch.cuda.current_stream(dev)
            custom = [_pairs_field(pair_list[i]) for i in members]
            explicit = any(p is not None for p in custom)
            side = None
            if (overlap and self.overlap_tail and tok is not None and tok.host_ids is None and tok.device == dev.index
                    and tok.stream == main.cuda_stream and tok.logits.data_ptr() == lg.data_ptr()
                    and tok.logits.numel() == lg.numel() and not quirk and not explicit
                    and all(pair_list[i].get_field("track_cls_logits").is_cuda for i in members)):
                side, ev_logits = self._side_stream(dev)
                side.wait_event(ev_logits)
                self._logits_token = None          # one decode per forward rides the event
            for i, p in zip(members, custom):
                rows = rel_logits[i].shape[0]
                if p is None and n * (n - 1) != rows:
                    raise ValueError(f"decode: segment {i}: rel_logits has {rows} rows but "
                                     f"{n} tracklets give {n * (n - 1)} pairs and no 'tracklet_pairs' field is set")
                if p is not None and tuple(p.shape) != (rows, 2):
                    raise ValueError(f"decode: segment {i}: 'tracklet_pairs' must be [P,2] with one row per "
                                     f"rel_logits row (P={rows}), got {tuple(p.shape)}")
            if explicit:
                pairs = torch.stack([ops.pair_index(n, dev) if p is None else p.to(dev) for p in custom]).contiguous()
            else:
                pairs = self._canonical_pairs(dev, nm, n)[1]
            if quirk:
                cls_src, row_mul = [pair_list[i].features for i in members], n - 1
            else:
                cls_src, row_mul = [pair_list[i].get_field("track_cls_logits") for i in members], 1
            with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
                # on the side stream the class logits are batched UNDER it: when they are not consecutive slices of
                # one allocation this is a cat / cast kernel, which on the caller's stream would sit behind the
                # whole encoder while the decode launch on the side stream read its (unwritten) result
                cls = _batch_rows(cls_src, dev).view((nm,) + tuple(cls_src[0].shape))
                res = ops.decode_topk(lg, pairs, cls, row_mul=row_mul, num_obj=num_obj, topk_per_pair=topk_per_pair,
                                      topk_per_seg=topk_per_seg, check_pairs=explicit)
            if side is not None:
                for r in res:
                    r.record_stream(main)          # allocated under the side stream, consumed on the caller's
                main.wait_stream(side)             # the caller's stream sees complete results from here on
            for k, i in enumerate(members):
                tgt = rel_logits[i].device
                out[i] = tuple(r[k].to(tgt) for r in res)
        return out

    def anchor_sizes(self, num_frames):
        """Anchor widths (frames) of the A anchors per location (DPN.anchor_sizes: the rule lives with the heads it
        parametrises, so that training from spans and decoding cannot disagree)."""
        return self.relpn.duration_proposal_network.anchor_sizes(num_frames)

    def decode_spans(self, duration_proposals, sizes=None, top_k=None, nms_threshold=0.5):
        """Temporal span proposals per pair from `forward`'s duration_proposals (span decode +
        temporal NMS on the GPU; completes the reference's stub RelNMS, rel_nms.py:5-15).
        Per segment a dict: anchor [P,k], span int64 [P,k,2] (frames [s,e)), span_f, score, count."""
        top_k = top_k or self.relpn.duration_proposal_network.top_k_proposals
        out = []
        for dp in duration_proposals:
            heads = dp.heads
            dev = _compute_device(heads)
            sz = sizes if sizes is not None else self.anchor_sizes(heads.shape[2])
            res = ops.decode_spans(_f32(heads, dev), sz, top_k=top_k, nms_threshold=nms_threshold)
            out.append({k: v.to(heads.device) for k, v in res.items()})
        return out

    def _cls_bf16(self, dev):
        """(classifier weight, bias) of the bf16 fused pass: fp32 tensors holding bf16-rounded values."""
        cls = self.classifier.rel_predictor
        return self.classifier._cache.get("cls_bf16", (cls.weight, cls.bias), dev,
                                          lambda ts: tuple(ops.cast_bf16(x.contiguous()).float() for x in ts))

    def _span_cls_bf16(self, dev):
        """(packed bf16 classifier of the bf16 span entries, its bias rounded to bf16 as fp32), cached beside "cls_bf16"."""
        cls = self.classifier.rel_predictor
        return self.classifier._cache.get(
            "cls_span_bf16", (cls.weight, cls.bias), dev,
            lambda ts: (ops.pack_span_cls_bf16(ts[0].contiguous()), ops.cast_bf16(ts[1].contiguous()).float()))

    def classify_spans(self, pair_list, spans):
        """Predicate logits with RelOIPool restricted to given spans: per segment `spans[i]` int64 [P,2]
        frames [start,end) (e.g. decode_spans(...)[i]["span"][:, j]); the build-defined meaning of
        RelOIPool.__call__(feats, duration_proposals) (reference model.py:68-73) + RelationPredictor.  A segment whose
        'tracklet_feats' are bf16 (D % 16 == 0) is pooled and classified with the bf16 semantics of `forward`
        (DESIGN.md §2): its logits equal forward's RELPN.DPN.POOL_TOP_SPAN logits for the same spans, bit for bit."""
        out = []
        with torch.no_grad():
            for plist, sp in zip(pair_list, spans):
                f = plist.get_field("tracklet_feats")
                dev = _compute_device(f, self.classifier.rel_predictor.weight)
                scorer = _scorer_kind(f)(self, dev, f.shape[2])
                p = _pairs_field(plist)
                p = ops.pair_index(f.shape[0], dev) if p is None else p.to(dev)
                sp = (sp if isinstance(sp, torch.Tensor) else torch.as_tensor(np.asarray(sp))).long().to(dev)
                out.append(scorer.span_logits(_batch_rows([f], dev, scorer.dtype), p.contiguous(), sp.contiguous()).to(f.device))
        return out

    def decode_span_relations(self, pair_list, duration_proposals, spans_per_pair=4, topk_per_span=20, topk_per_seg=200,
                              num_obj=35, sizes=None, nms_threshold=0.5):
        """Relations WITH their temporal spans from `forward`'s duration_proposals (build-defined): per
        pair the `spans_per_pair` best span proposals (`decode_spans`), per span the `topk_per_span` best predicates of
        the predicate head pooled over that span, scored predicate sigmoid x span relationness, and per segment the
        `topk_per_seg` best of those.  Per segment returns (scores [M], triplets int64 [M,3] = (subject class,
        predicate, object class), pair_tids int64 [M,2], spans int64 [M,2] frames [start, end) inside the segment), in
        descending score order, on the device of the segment's 'tracklet_feats'.  Needs the tracklet fields
        ('tracklet_feats' [N,T,D], 'track_cls_logits' [N,num_obj]); honours 'tracklet_pairs'.  Segments with fewer than
        2 tracklets or no pair yield empty results.  Equal-shape segments of one feature dtype share one launch; bf16
        'tracklet_feats' (D % 16 == 0) take the bf16 entries and semantics; everything runs on the caller's stream."""
        cls = self.classifier.rel_predictor
        out = [None] * len(pair_list)
        groups = {}
        with torch.no_grad():
            for i, (plist, dp) in enumerate(zip(pair_list, duration_proposals)):
                if not self._is_tracklet_sample(plist):
                    raise ValueError(f"decode_span_relations: segment {i} has no 'tracklet_feats': spans need temporal features")
                f = plist.get_field("tracklet_feats")
                n = int(f.shape[0])
                heads = dp.heads
                if n <= 1 or heads.shape[0] == 0:
                    tgt = f.device
                    out[i] = (torch.empty(0, device=tgt), torch.empty((0, 3), dtype=torch.int64, device=tgt),
                              torch.empty((0, 2), dtype=torch.int64, device=tgt), torch.empty((0, 2), dtype=torch.int64, device=tgt))
                    continue
                c = plist.get_field("track_cls_logits")
                if tuple(c.shape) != (n, num_obj):
                    raise ValueError(f"decode_span_relations: segment {i}: 'track_cls_logits' must be [{n},{num_obj}], got {tuple(c.shape)}")
                groups.setdefault((tuple(f.shape), tuple(heads.shape), _scorer_kind(f)), []).append(i)
            for (fshape, hshape, kind), members in groups.items():
                n, nm = fshape[0], len(members)
                dev = _compute_device(*[pair_list[i].get_field("tracklet_feats") for i in members], cls.weight)
                scorer = kind(self, dev, fshape[2])
                pairs = []
                for i in members:
                    p = _segment_pairs(pair_list[i], n, dev)
                    if p.shape[0] != hshape[0]:
                        raise ValueError(f"decode_span_relations: segment {i}: {p.shape[0]} pairs but duration_proposals "
                                         f"has {hshape[0]} rows")
                    pairs.append(p)
                pairs = torch.stack(pairs).contiguous()
                heads = _batch_rows([duration_proposals[i].heads for i in members], dev)
                sz = sizes if sizes is not None else self.anchor_sizes(hshape[2])
                sp = ops.decode_spans(heads, sz, top_k=spans_per_pair, nms_threshold=nms_threshold)
                feats = _batch_rows([pair_list[i].get_field("tracklet_feats") for i in members], dev, scorer.dtype)
                clog = _batch_rows([pair_list[i].get_field("track_cls_logits") for i in members], dev).view(nm, n, num_obj)
                res = scorer.span_relations(feats, pairs, sp, clog, topk_per_span, topk_per_seg)
                valid = res[5].tolist()
                for k, i in enumerate(members):
                    tgt = pair_list[i].get_field("tracklet_feats").device
                    out[i] = tuple(r[k, :valid[k]].to(tgt) for r in res[:4])
        return out

    def pair_geometry(self, pair_list):
        """Relative box geometry [P,8,T] per segment from 'tracklet_boxes' (pair builder side output)."""
        out = []
        for plist in pair_list:
            boxes = plist.get_field("tracklet_boxes")
            dev = _compute_device(boxes)
            n = boxes.shape[0]
            _, g = ops.pair_gather(None, _f32(boxes, dev), ops.pair_index(n, dev), want_feat=False)
            out.append(g.to(boxes.device))
        return out
