"""Tensor-level wrappers over the C ABI (device tensors in, device tensors out).

PyTorch is plumbing here: it owns HBM allocations and the HIP stream; every
operator below runs in the hand-written HIP library.  Inputs must already be
fp32 / int64, contiguous, on a HIP device — anything else raises; there is no
CPU path.
"""
import ctypes
import threading

import torch

from . import _abi

__all__ = [
    "predicate_head", "feature_preprocess_", "ppn_pair_matrix_topk", "traj_iou", "traj_iou_tail", "pair_index",
    "pair_gather", "pack_conv3", "conv3", "conv3_tc", "pack_conv3_wino63", "conv3_tc_wino63", "pack_conv3_wino63_f16x3", "conv3_tc_wino63_f16x3", "heads", "heads_pairgrid", "heads_pairgrid_f16x3", "heads_pairgrid_f16x3_split_bytes",
    "heads_pairgrid_f16x3_set_force_exact", "heads_pair_f16x3_set_diag_skip","temporal_mean", "temporal_sum", "pair_rows", "transpose_td",
    "forward_fused", "temporal_encoder_heads", "fused_workspace_bytes", "fused_bf16_workspace_bytes", "decode_topk", "decode_spans", "decode_span_relations",
    "span_anchor_labels", "span_loss", "span_anchor_sample", "pair_labels", "span_match",
    "span_labels", "span_predicate_loss", "span_predicate_grad",
    "cast_bf16", "pack_conv3_bf16", "pack_heads_bf16", "conv3_tc_bf16", "heads_pairgrid_bf16",
    "pair_plan", "heads_pairlist_bf16",
    "transpose_cast_bf16", "temporal_encoder_heads_bf16",
    "temporal_mean_bf16", "forward_fused_bf16", "span_predicate",
    "pack_span_cls_bf16", "span_predicate_bf16", "decode_span_relations_bf16", "bottleneck_block_bf16", "bottleneck_block_proj_bf16", "bottleneck_block_res_bf16",
    "proposal_pair_filter", "gather_rows", "wino63_set_piece_form", "wino63_f16x3_set_tail_split", "conv3_spot_check",
    "wino63_f16x3_set_input_form", "wino63_f16x3_input_form", "wino63_f16x3_input",
    "pack_conv2d", "pack_conv2d_frag", "conv2d_nhwc", "roi_align_nhwc", "pack_conv2d_frag_bf16", "conv2d_nhwc_bf16", "max_pool_nhwc", "pack_conv2d_frag_cin4", "conv2d_nhwc_cin4", "max_pool_nhwc_bf16", "pack_stem_bf16", "stem_conv_bf16", "stem_pool_bf16", "bottleneck_tail_bf16",
    "eval_traj_volume", "eval_viou", "eval_greedy_match", "evalobj_tiou", "evalobj_claim",
    "rpn_decode", "box_head_decode", "box_nms", "box_nms_workspace_bytes", "detections_topk", "rpn_proposals", "box_detections",
    "link_detections", "link_fill",
    "status_words", "status_fault", "status_clear", "status_selftest",
]


_status_blocks = {}          # device index -> numpy view of the pinned int32 [STATUS_WORDS] the kernels of that device can write
_status_lock = threading.Lock()


def _status_block(index=None):
    """The device status block of device `index` (default: the current one), allocated and attached on first use:
    `_abi.STATUS_WORDS` int32 of pinned host memory (include/tspn_mi355x.h, "device status block").  A kernel that
    detects a fault raises it there; the next launch entry of the library then returns TSPN_EDEVICE, which
    `_abi.check` turns into a `TspnError` -- without any synchronisation."""
    idx = torch.cuda.current_device() if index is None else int(index)
    blk = _status_blocks.get(idx)
    if blk is not None:
        return blk
    with _status_lock:
        blk = _status_blocks.get(idx)
        if blk is None:
            raw = torch.zeros(_abi.STATUS_WORDS + 16, dtype=torch.int32).pin_memory()
            off = (-(raw.data_ptr() // 4)) % 16                     # 64-byte aligned
            blk = raw[off:off + _abi.STATUS_WORDS]
            with torch.cuda.device(idx):
                _abi.check(_abi.lib().tspn_status_attach(ctypes.c_void_p(blk.data_ptr())))
            blk = _status_blocks[idx] = blk.numpy()             # live view of the pinned words (it keeps the tensor alive)
    return blk


def _stream():
    """Current stream of the CURRENT device; every public op runs under `_on_tensor_device`, which makes
    the device of its tensor arguments current for the duration of the call.  Every launch passes here: the
    device's status block is attached before its first kernel runs."""
    blk = _status_block()
    # fail fast: with a fault standing on this device nothing more is launched from here (the C entries report it too, but
    # only where they check the launch error, i.e. after enqueueing their kernel)
    fault = int(blk[_abi.STATUS_FAULT])
    if fault:
        raise _abi.TspnError(_abi.TSPN_EDEVICE,
                             f"device {torch.cuda.current_device()} reported fault 0x{fault:x}"
                             + (" (an LDS hand-over between waves timed out)" if fault & _abi.FAULT_HANDOVER else "")
                             + f", info 0x{int(blk[_abi.STATUS_FAULT_INFO]) & 0xffffffff:x}, in an earlier launch of this library: "
                             "results produced since are not to be trusted; ops.status_clear() re-arms")
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def status_words(device=None):
    """Live numpy view of a device's status block (words: _abi.STATUS_*)."""
    return _status_block(None if device is None else torch.device(device).index)


def status_fault(device=None):
    """The fault word of a device (0 = healthy), read from pinned host memory: no synchronisation."""
    return int(status_words(device)[_abi.STATUS_FAULT])


def status_clear(device=None):
    """Re-arm after a fault has been dealt with (results since the fault are not to be trusted)."""
    w = status_words(device)
    w[_abi.STATUS_FAULT_INFO] = 0
    w[_abi.STATUS_FAULT] = 0


def status_selftest(device=None):
    """Raise TSPN_FAULT_HANDOVER on purpose, through the device code of the role-split res4 tail's bounded wait
    (tspn_status_selftest).  Returns a device int32 that stays 0: the wave ends inside the wait."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        reached = torch.zeros(1, dtype=torch.int32, device=dev)
        _status_block()
        _abi.check(_abi.lib().tspn_status_selftest(_p(reached), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return reached


def _first_hip_device(obj, depth=0):
    if isinstance(obj, torch.Tensor):
        return obj.device if obj.is_cuda else None
    if depth < 2:
        if isinstance(obj, (list, tuple)):
            for v in obj:
                d = _first_hip_device(v, depth + 1)
                if d is not None:
                    return d
        elif isinstance(obj, dict):
            for v in obj.values():
                d = _first_hip_device(v, depth + 1)
                if d is not None:
                    return d
    return None


def _on_tensor_device(fn):
    """The C ABI launches on the stream it is handed and never calls hipSetDevice; kernels, the
    per-device LDS limits and the workspace allocations of an op must all belong to the device that
    holds its operands.  This wrapper makes that device current (a no-op when it already is) and
    refuses operands spread over several devices."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        dev = None
        for a in list(args) + list(kwargs.values()):
            d = _first_hip_device(a)
            if d is None:
                continue
            if dev is None:
                dev = d
            elif d != dev:
                raise RuntimeError(f"{fn.__name__}: operands live on different devices ({dev} and {d})")
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapper


def _dev(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: tensor is on {t.device}; the TSPN HIP path needs a HIP device "
                           "tensor (there is no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: tensor must be contiguous")
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _ws(nbytes, device):
    # torch's caching allocator returns >= 256-B aligned blocks
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _workspace(workspace, need, device, who, sizes=False):
    """The caller's `workspace` if it holds `need` bytes (`sizes`: the refusal names both numbers), or a new one from the
    module's `_ws`, looked up at call time.  A buffer allocated here is not measured: whether it is large enough is the C
    entry's TSPN_EWORKSPACE to say."""
    if workspace is None:
        return _ws(need, device)
    if workspace.numel() * workspace.element_size() < need:
        raise ValueError(f"{who}: workspace too small" + (f" ({workspace.numel()} < {need})" if sizes else ""))
    return workspace


def _toggle(setter, value):
    """Set a process-wide switch of the library (a tspn_*_set_* entry); returns the previous setting."""
    prev = getattr(_abi.lib(), setter)(int(value))
    if prev < 0:
        _abi.check(prev)
    return prev


def _out_hw(who, H, W, KH, KW, stride, padding):
    """(OH, OW) of a KH x KW window over an H x W map; an empty output is refused."""
    OH, OW = (H + 2 * padding - KH) // stride + 1, (W + 2 * padding - KW) // stride + 1
    if OH <= 0 or OW <= 0:
        raise ValueError(f"{who}: empty output")
    return OH, OW


def predicate_head(x, weight, bias, apply_sigmoid=True, norm=None):
    """sigmoid(x @ W.T + b) — RelationPredictor.forward (reference lib/modeling/model.py:85-88).

    `norm=(first, block, nblocks)`: x holds RAW features and the block-L1 normalisation of
    VRDataset._feature_preprocess (lib/dataset/vrdataset.py:219-243) is folded into the GEMM."""
    _dev(x, "x"); _dev(weight, "weight")
    if bias is not None:
        _dev(bias, "bias")
    if x.dim() != 2 or weight.dim() != 2 or x.shape[1] != weight.shape[1]:
        raise ValueError(f"predicate_head: shapes {tuple(x.shape)} x {tuple(weight.shape)}^T do not match")
    if bias is not None and bias.shape != (weight.shape[0],):
        raise ValueError("predicate_head: bias shape mismatch")
    P, F = x.shape
    K = weight.shape[0]
    out = torch.empty((P, K), dtype=torch.float32, device=x.device)
    l = _abi.lib()
    if norm is not None:
        first, block, nblocks = (int(v) for v in norm)
        if first < 0 or block <= 0 or nblocks < 0 or first + block * nblocks > F:
            raise ValueError(f"predicate_head: normalisation blocks {norm} exceed F={F}")
        ws = _ws(l.tspn_predicate_head_norm_workspace_bytes(P, F, K, first, block, nblocks), x.device)
        _abi.check(l.tspn_predicate_head_norm_f32(_p(x), P, F, F, _p(weight), _p(bias), K, first, block,
                                                  nblocks, _p(out), 1 if apply_sigmoid else 0, _p(ws),
                                                  ws.numel(), _stream()))
        return out
    nbytes = l.tspn_predicate_head_workspace_bytes(P, F, K)
    ws = _ws(nbytes, x.device)
    _abi.check(l.tspn_predicate_head_f32(_p(x), P, F, F, _p(weight), _p(bias), K, _p(out),
                                         1 if apply_sigmoid else 0, _p(ws), ws.numel(), _stream()))
    return out


def feature_preprocess_(feats, first=70, block=1000, nblocks=8):
    """In-place block-L1 normalisation — VRDataset._feature_preprocess (lib/dataset/vrdataset.py:219-243)."""
    _dev(feats, "feats")
    if feats.dim() != 2:
        raise ValueError("feature_preprocess_: feats must be [P,F]")
    P, F = feats.shape
    _abi.check(_abi.lib().tspn_feature_preprocess_f32(_p(feats), P, F, F, first, block, nblocks, _stream()))
    return feats


def proposal_pair_filter(pairs, trackid, pair_off=None, track_off=None):
    """VRDataset._get_proposal_idx + _get_num_tracklet_proposals (lib/dataset/vrdataset.py:140-148).

    One segment: pairs int64 [P,2] (track indices as stored in the -relation.h5 file), trackid int64 [M]
    (-1 = proposal, >= 0 = ground truth) -> (proposal_idx int64 [P'], num_tracks int).
    Several segments stored back to back: pass int64 offsets pair_off [S+1], track_off [S+1] (device
    tensors) -> (idx int64 [P_total] with segment s's kept local indices at idx[pair_off[s]:pair_off[s]
    + count[s]], count int64 [S], num_tracks int64 [S]) as device tensors (no host sync).
    A pair naming a track outside its segment raises IndexError (single-segment form) or yields
    count -1 (batched form)."""
    _dev(pairs, "pairs", torch.int64); _dev(trackid, "trackid", torch.int64)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or trackid.dim() != 1:
        raise ValueError("proposal_pair_filter: pairs must be [P,2] and trackid [M]")
    dev = pairs.device
    single = pair_off is None
    if single:
        pair_off = torch.tensor([0, pairs.shape[0]], dtype=torch.int64, device=dev)
        track_off = torch.tensor([0, trackid.shape[0]], dtype=torch.int64, device=dev)
    _dev(pair_off, "pair_off", torch.int64); _dev(track_off, "track_off", torch.int64)
    if pair_off.shape != track_off.shape or pair_off.dim() != 1 or pair_off.numel() < 1:
        raise ValueError("proposal_pair_filter: pair_off / track_off must be int64 [S+1]")
    S = pair_off.numel() - 1
    idx = torch.empty((pairs.shape[0],), dtype=torch.int64, device=dev)
    count = torch.empty((S,), dtype=torch.int64, device=dev)
    ntr = torch.empty((S,), dtype=torch.int64, device=dev)
    _abi.check(_abi.lib().tspn_proposal_pair_filter_i64(_p(pairs), _p(pair_off), _p(trackid), _p(track_off), S,
                                                        _p(idx), _p(count), _p(ntr), _stream()))
    if not single:
        return idx, count, ntr
    c = int(count[0])
    if c < 0:
        raise IndexError("proposal_pair_filter: a pair names a track index outside trackid")
    return idx[:c], int(ntr[0])


def gather_rows(src, idx, check_idx=True):
    """out[r] = src[idx[r]] for a 2-D fp32 matrix (feats[proposal_idx], lib/dataset/vrdataset.py:66-67).
    `check_idx=False` skips the range check (two host syncs) for indices a kernel of this library produced
    (proposal_pair_filter emits range-checked local row numbers)."""
    _dev(src, "src"); _dev(idx, "idx", torch.int64)
    if src.dim() != 2 or idx.dim() != 1:
        raise ValueError("gather_rows: src must be [R,F] and idx [R']")
    if check_idx and idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= src.shape[0]):
        raise IndexError("gather_rows: row index out of range")
    out = torch.empty((idx.numel(), src.shape[1]), dtype=torch.float32, device=src.device)
    if src.shape[1]:
        _abi.check(_abi.lib().tspn_gather_rows_f32(_p(src), src.shape[1], src.shape[1], _p(idx), 0, idx.numel(),
                                                   _p(out), _stream()))
    return out


def ppn_pair_matrix_topk(cls_logits, w, topk):
    """PPNHead + top-k (lib/modeling/relpn/ppn.py:107-112, 84-85).

    cls_logits [B,N,Cin] or [N,Cin]; `w` = dict with keys sub_emb.0.weight ... obj_emb.2.bias.
    Returns (pair_matrix [B,N,N], idx int64 [B,min(topk,N*N)]) (batch dim dropped for 2-D input).

    Capacity: one workgroup holds a segment in LDS, 4*N*(Cin+H+2*Cout) + 8*n2p bytes (n2p = N*N rounded up to a power
    of two) against 160 KiB.  At the model's widths (35, 64, 35) the largest N is 90; N = 91 ... 128 raise
    TSPN_EUNSUPPORTED (the message names LDS).  N = 128 runs only with narrow embeddings, e.g. H = Cout = 8.
    """
    squeeze = cls_logits.dim() == 2
    c = cls_logits.unsqueeze(0) if squeeze else cls_logits
    _dev(c, "cls_logits")
    B, N, Cin = c.shape
    ks = ["sub_emb.0.weight", "sub_emb.0.bias", "sub_emb.2.weight", "sub_emb.2.bias",
          "obj_emb.0.weight", "obj_emb.0.bias", "obj_emb.2.weight", "obj_emb.2.bias"]
    ts = [_dev(w[k], k) for k in ks]
    H, Cout = ts[0].shape[0], ts[2].shape[0]
    if ts[0].shape != (H, Cin) or ts[2].shape != (Cout, H) or ts[4].shape != (H, Cin) or ts[6].shape != (Cout, H):
        raise ValueError("ppn_pair_matrix_topk: weight shapes do not match the input")
    k = min(int(topk), N * N)
    mat = torch.empty((B, N, N), dtype=torch.float32, device=c.device)
    idx = torch.empty((B, k), dtype=torch.int64, device=c.device)
    _abi.check(_abi.lib().tspn_ppn_pair_matrix_topk_f32(
        _p(c), B, N, Cin, H, Cout, *[_p(t) for t in ts], k, _p(mat), _p(idx), _stream()))
    return (mat[0], idx[0]) if squeeze else (mat, idx)


def traj_iou(boxes1, boxes2=None):
    """cubic_iou (lib/modeling/trajectory.py:127-141); boxes [N,T,4] or [B,N,T,4] -> [.., N1, N2]."""
    squeeze = boxes1.dim() == 3
    b1 = boxes1.unsqueeze(0) if squeeze else boxes1
    _dev(b1, "boxes1")
    B, N1, T, four = b1.shape
    if four != 4:
        raise ValueError("traj_iou: last dim must be 4")
    if boxes2 is None:
        b2, N2 = None, N1
    else:
        b2 = boxes2.unsqueeze(0) if squeeze else boxes2
        _dev(b2, "boxes2")
        if b2.shape[0] != B or b2.shape[2] != T or b2.shape[3] != 4:
            raise ValueError("traj_iou: boxes2 shape mismatch")
        N2 = b2.shape[1]
    out = torch.empty((B, N1, N2), dtype=torch.float32, device=b1.device)
    if out.numel() == 0:      # an empty boxes2 has a null data pointer, which the C entry reads as "self-IoU"
        return out[0] if squeeze else out
    _abi.check(_abi.lib().tspn_traj_iou_f32(_p(b1), N1, _p(b2), N2, B, T, _p(out), _stream()))
    return out[0] if squeeze else out


@_on_tensor_device
def traj_iou_tail(a, len_a, b, out=None):
    """Association-time IoU, one launch per segment (replaces the per-candidate `_traj_iou` calls of reference
    lib/modeling/association.py:35-48,101-106): a [U,L,4] float64 = trajectories from the segment's first frame on,
    len_a [U] int32 = their number of common frames (<= L; 0 -> IoU 0), b [N,L,4] float64 = the segment's tracklets
    -> [U,N] float32 with the reference chain's roundings (tspn_traj_iou_tail_f64)."""
    _dev(a, "a", torch.float64), _dev(b, "b", torch.float64), _dev(len_a, "len_a", torch.int32)
    if a.dim() != 3 or b.dim() != 3 or a.shape[2] != 4 or b.shape[2] != 4 or a.shape[1] != b.shape[1]:
        raise ValueError(f"traj_iou_tail: a [U,L,4] and b [N,L,4] expected, got {tuple(a.shape)} and {tuple(b.shape)}")
    U, L, _ = a.shape
    N = b.shape[0]
    if len_a.shape != (U,):
        raise ValueError(f"traj_iou_tail: len_a must be [{U}], got {tuple(len_a.shape)}")
    if not (a.is_contiguous() and b.is_contiguous() and len_a.is_contiguous()):
        raise ValueError("traj_iou_tail: operands must be contiguous")
    if out is None:
        out = torch.empty((U, N), dtype=torch.float32, device=a.device)
    elif out.shape != (U, N) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != a.device:
        raise ValueError("traj_iou_tail: out must be a contiguous float32 [U,N] tensor on the operands' device")
    _abi.check(_abi.lib().tspn_traj_iou_tail_f64(_p(a), _p(len_a), _p(b), U, N, L, _p(out), _stream()))
    return out


def pair_index(n, device, base=0):
    """All ordered pairs (i,j), i != j, i-major (lib/modeling/predict.py:133-140), int64 [n(n-1), 2]."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("pair_index: needs a HIP device (no CPU fallback)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        out = torch.empty((max(n * (n - 1), 0), 2), dtype=torch.int64, device=dev)
        _abi.check(_abi.lib().tspn_pair_index_i64(n, base, _p(out), _stream()))
    return out


def pair_gather(tracklet_feats, tracklet_boxes, pairs, want_feat=True, want_geom=True, check_pairs=True, out_geom=None):
    """N^2 pair builder: -> (pair_feats [P,2D,T] | None, pair_geom [P,8,T] | None).  `out_geom`: caller-held
    contiguous fp32 [P,8,T] the geometry is written into (e.g. a slice of a buffer another stream reads later)."""
    _dev(pairs, "pairs", torch.int64)
    P = pairs.shape[0]
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError("pair_gather: pairs must be [P,2]")
    feat = geom = None
    NT = T = D = None
    if want_feat:
        _dev(tracklet_feats, "tracklet_feats")
        NT, T, D = tracklet_feats.shape
        feat = torch.empty((P, 2 * D, T), dtype=torch.float32, device=pairs.device)
    if want_geom:
        _dev(tracklet_boxes, "tracklet_boxes")
        if tracklet_boxes.dim() != 3 or tracklet_boxes.shape[2] != 4:
            raise ValueError("pair_gather: tracklet_boxes must be [N,T,4]")
        if NT is not None and tuple(tracklet_boxes.shape[:2]) != (NT, T):
            raise ValueError("pair_gather: feats / boxes shape mismatch")
        NT, T = tracklet_boxes.shape[:2]
        if out_geom is None:
            geom = torch.empty((P, _abi.GEOM_CHANNELS, T), dtype=torch.float32, device=pairs.device)
        else:
            _dev(out_geom, "out_geom")
            if tuple(out_geom.shape) != (P, _abi.GEOM_CHANNELS, T):
                raise ValueError(f"pair_gather: out_geom must be [{P},{_abi.GEOM_CHANNELS},{T}], got {tuple(out_geom.shape)}")
            geom = out_geom
        D = D or 1
    if NT is None:
        return None, None
    if check_pairs and P and (int(pairs.min()) < 0 or int(pairs.max()) >= NT):   # host sync: skip for tables built here
        raise IndexError("pair_gather: pair index out of range")
    _abi.check(_abi.lib().tspn_pair_gather_f32(
        _p(tracklet_feats if want_feat else None), _p(tracklet_boxes if want_geom else None),
        NT, T, D, _p(pairs), P, _p(feat), _p(geom), _stream()))
    return feat, geom


def pack_conv3(weight, split=0):
    """nn.Conv1d weight [M,Cin,3] -> MFMA staging layout [3][Cin'][M'] (see tspn_pack_conv3_f32)."""
    _dev(weight, "conv weight")
    if weight.dim() != 3 or weight.shape[2] != 3:
        raise ValueError("pack_conv3: weight must be [M,Cin,3]")
    M, Cin, _ = weight.shape
    if split:
        shape = (3, split, 2 * M)
    else:
        shape = (3, Cin, M)
    packed = torch.empty(shape, dtype=torch.float32, device=weight.device)
    _abi.check(_abi.lib().tspn_pack_conv3_f32(_p(weight), M, Cin, split, _p(packed), _stream()))
    return packed


def conv3(x, packed, bias=None, relu=False):
    """y[B,M,T] = act(bias + conv1d_k3(x[B,Cin,T])) with packed weights [3,Cin,M]."""
    _dev(x, "x"); _dev(packed, "packed")
    if bias is not None:
        _dev(bias, "bias")
    B, Cin, T = x.shape
    if packed.dim() != 3 or packed.shape[0] != 3 or packed.shape[1] != Cin:
        raise ValueError(f"conv3: packed weights {tuple(packed.shape)} do not match Cin={Cin}")
    M = packed.shape[2]
    if bias is not None and bias.shape != (M,):
        raise ValueError("conv3: bias shape mismatch")
    y = torch.empty((B, M, T), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().tspn_conv3_f32(_p(x), B, Cin, T, _p(packed), M, _p(bias), 1 if relu else 0,
                                         _p(y), _stream()))
    return y


def conv3_tc(x, packed, bias=None, relu=False):
    """conv3 on channels-last x[B,T,Cin] (tracklet layout) -> y[B,M,T]; fast path only."""
    _dev(x, "x"); _dev(packed, "packed")
    if bias is not None:
        _dev(bias, "bias")
    B, T, Cin = x.shape
    if packed.dim() != 3 or packed.shape[0] != 3 or packed.shape[1] != Cin:
        raise ValueError(f"conv3_tc: packed weights {tuple(packed.shape)} do not match Cin={Cin}")
    M = packed.shape[2]
    y = torch.empty((B, M, T), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().tspn_conv3_tc_f32(_p(x), B, T, Cin, _p(packed), M, _p(bias), 1 if relu else 0,
                                            _p(y), _stream()))
    return y


def wino63_frag_dims(frag):
    """(Cin, M) of a fragment-major F(6,3) weight tensor (pack_conv3_wino63)."""
    if frag.dim() != 5 or tuple(frag.shape[2:]) != (8, 64, 4):
        raise ValueError(f"not a fragment-major F(6,3) weight tensor: {tuple(frag.shape)}")
    return frag.shape[1] * 8, frag.shape[0] * 32


def pack_conv3_wino63(weight, split=0):
    """nn.Conv1d weight [M,Cin,3] -> Winograd F(6,3) weights, fragment-major [M'/32][Cin'/8][8][64][4]
    (tspn_pack_conv3_wino63_frag_f32; split as in pack_conv3).  Needs Cin' % 8 == 0, M' % 32 == 0."""
    _dev(weight, "conv weight")
    if weight.dim() != 3 or weight.shape[2] != 3:
        raise ValueError("pack_conv3_wino63: weight must be [M,Cin,3]")
    M, Cin, _ = weight.shape
    Mp, Cp = (2 * M, split) if split else (M, Cin)
    if Cp % 8 or Mp % 32:
        raise ValueError(f"pack_conv3_wino63: needs Cin % 8 == 0 and M % 32 == 0 (Cin={Cp}, M={Mp})")
    frag = torch.empty((Mp // 32, Cp // 8, 8, 64, 4), dtype=torch.float32, device=weight.device)
    _abi.check(_abi.lib().tspn_pack_conv3_wino63_frag_f32(_p(weight), M, Cin, split, _p(frag), _stream()))
    return frag


def conv3_tc_wino63(x, frag, bias=None, relu=False, workspace=None):
    """Winograd F(6,3) conv3 (tspn_wino63.hip): channels-last x[B,T,Cin] with pack_conv3_wino63 weights -> y[B,M,T].
    Needs Cin % 32 == 0; `workspace` (uint8, >= tspn_conv3_tc_wino63_workspace_bytes) holds the transformed input."""
    _dev(x, "x"); _dev(frag, "frag")
    if bias is not None:
        _dev(bias, "bias")
    B, T, Cin = x.shape
    cin_w, M = wino63_frag_dims(frag)
    if cin_w != Cin:
        raise ValueError(f"conv3_tc_wino63: weights are for Cin={cin_w}, x has Cin={Cin}")
    l = _abi.lib()
    need = l.tspn_conv3_tc_wino63_workspace_bytes(B, T, Cin)
    workspace = _workspace(workspace, need, x.device, "conv3_tc_wino63", sizes=True)
    y = torch.empty((B, M, T), dtype=torch.float32, device=x.device)
    _abi.check(l.tspn_conv3_tc_wino63_f32(_p(x), B, T, Cin, _p(frag), M, _p(bias), 1 if relu else 0, _p(y),
                                          _p(workspace), workspace.numel() * workspace.element_size(), _stream()))
    return y


def wino63_f16x3_dims(packed):
    """(Cin, M) of a split-fp16 F(6,3) weight tensor (pack_conv3_wino63_f16x3)."""
    if packed.dim() != 4 or packed.dtype != torch.int16 or packed.shape[0] != 8 or packed.shape[3] != 8 \
            or packed.shape[1] % 2 != 1:
        raise ValueError(f"not a split-fp16 F(6,3) weight tensor: {tuple(packed.shape)} {packed.dtype}")
    return (packed.shape[1] - 1) // 2 * 8, packed.shape[2]


def pack_conv3_wino63_f16x3(weight, split=0):
    """nn.Conv1d weight [M,Cin,3] -> split-fp16 Winograd F(6,3) weights (tspn_pack_conv3_wino63_f16x3; split as in
    pack_conv3): int16 storage [8 points][2 Cin'/8 + 1][M'][8] = fp16 hi parts, lo parts and one exponent slot per row.
    Needs Cin' % 32 == 0, M' % 256 == 0."""
    _dev(weight, "conv weight")
    if weight.dim() != 3 or weight.shape[2] != 3:
        raise ValueError("pack_conv3_wino63_f16x3: weight must be [M,Cin,3]")
    M, Cin, _ = weight.shape
    Mp, Cp = (2 * M, split) if split else (M, Cin)
    if Cp % 32 or Mp % 256:
        raise ValueError(f"pack_conv3_wino63_f16x3: needs Cin % 32 == 0 and M % 256 == 0 (Cin={Cp}, M={Mp})")
    packed = torch.empty((8, 2 * (Cp // 8) + 1, Mp, 8), dtype=torch.int16, device=weight.device)
    assert packed.numel() == _abi.lib().tspn_pack_conv3_wino63_f16x3_elements(M, Cin, split)
    _abi.check(_abi.lib().tspn_pack_conv3_wino63_f16x3(_p(weight), M, Cin, split, _p(packed), _stream()))
    return packed


def conv3_tc_wino63_f16x3(x, packed, bias=None, relu=False, workspace=None):
    """Split-fp16 Winograd F(6,3) conv3 (tspn_conv3_tc_wino63_f16x3): channels-last x[B,T,Cin] with
    pack_conv3_wino63_f16x3 weights -> y[B,M,T].  `workspace` (uint8, >= tspn_conv3_tc_wino63_f16x3_workspace_bytes)."""
    _dev(x, "x")
    if bias is not None:
        _dev(bias, "bias")
    B, T, Cin = x.shape
    cin_w, M = wino63_f16x3_dims(packed)
    if cin_w != Cin:
        raise ValueError(f"conv3_tc_wino63_f16x3: weights are for Cin={cin_w}, x has Cin={Cin}")
    l = _abi.lib()
    need = l.tspn_conv3_tc_wino63_f16x3_workspace_bytes(B, T, Cin, M)
    workspace = _workspace(workspace, need, x.device, "conv3_tc_wino63_f16x3", sizes=True)
    y = torch.empty((B, M, T), dtype=torch.float32, device=x.device)
    _abi.check(l.tspn_conv3_tc_wino63_f16x3(_p(x), B, T, Cin, _p(packed), M, _p(bias), 1 if relu else 0, _p(y),
                                            _p(workspace), workspace.numel() * workspace.element_size(), _stream()))
    return y


def wino63_set_piece_form(form):
    """0 = buffer-load pieces where the operands allow (default), 1 = 64-bit pointer pieces everywhere, for the fp32
    and the split-fp16 F(6,3) contraction (tspn_conv3_tc_wino63_set_piece_form).  Returns the previous setting."""
    return _toggle("tspn_conv3_tc_wino63_set_piece_form", form)


def wino63_f16x3_set_tail_split(on):
    """1 = the split-fp16 contraction cuts the tiles of its last, partly filled round into sub-tiles (default), 0 = whole
    tiles only (tspn_conv3_tc_wino63_f16x3_set_tail_split); same outputs bit for bit.  Returns the previous setting."""
    return _toggle("tspn_conv3_tc_wino63_f16x3_set_tail_split", on)


def wino63_f16x3_set_input_form(form):
    """Which kernels run ahead of the split-fp16 F(6,3) contraction (tspn_conv3_tc_wino63_f16x3_set_input_form): 0 = chosen
    by shape (default, `wino63_f16x3_input_form`), 1 = the two-pass transform (and the mean kernel) everywhere, 2 = the
    fused kernels (column maxima and mean in one read) wherever they support the shape; same outputs bit for bit.  Returns the previous setting."""
    return _toggle("tspn_conv3_tc_wino63_f16x3_set_input_form", form)


def wino63_f16x3_input_form(NT, T, Cin, cus):
    """1 where the default takes the fused input kernels for NT tracklets [T, Cin] on a device of `cus` compute units,
    else 0 (tspn_conv3_tc_wino63_f16x3_input_form: a pure host function, no device needed)."""
    return int(_abi.lib().tspn_conv3_tc_wino63_f16x3_input_form(int(NT), int(T), int(Cin), int(cus)))


def wino63_f16x3_input(x, M, workspace=None, mean=True, hot=True):
    """The input side of the split-fp16 F(6,3) conv alone (tspn_conv3_tc_wino63_f16x3_input) on channels-last x[B,T,Cin]
    for M output rows.  Returns (v, e, fbar, key): the split input as int16 [8, 2, Cin/8, nsp2, 8], the column exponents
    int32 [8, nsp2] (both views of the workspace), the temporal mean [B, Cin] or None, and the hot-sextet key
    ((float bits of the largest |x| << 32) | sextet) as a 0-d int64 tensor or None."""
    _dev(x, "x")
    B, T, Cin = x.shape
    l = _abi.lib()
    need = l.tspn_conv3_tc_wino63_f16x3_workspace_bytes(B, T, Cin, M)
    workspace = _workspace(workspace, need, x.device, "wino63_f16x3_input", sizes=True)
    fbar = torch.empty((B, Cin), dtype=torch.float32, device=x.device) if mean else None
    slots = torch.zeros((64, 32), dtype=torch.int64, device=x.device) if hot else None
    _abi.check(l.tspn_conv3_tc_wino63_f16x3_input(_p(x), B, T, Cin, M, _p(workspace),
                                                  workspace.numel() * workspace.element_size(), _p(fbar), _p(slots), _stream()))
    nsp2 = -(-(B * (-(-T // 6))) // 256) * 256
    vbytes = 8 * 2 * Cin * nsp2 * 2
    v = workspace[:vbytes].view(torch.int16).view(8, 2, Cin // 8, nsp2, 8)
    eoff = -(-vbytes // 256) * 256
    e = workspace[eoff:eoff + 8 * nsp2 * 4].view(torch.int32).view(8, nsp2)
    return v, e, fbar, (slots[:, 0].max() if hot else None)


def heads(a, head_w, head_b, b=None, ia=None, ib=None, bias=None, channels=None, num_pairs=None):
    """out[P,H,T] = head_b + head_w @ h_p; h_p = a[ia[p]] (dense) or relu(a[ia[p]] + b[ib[p]] + bias)."""
    _dev(a, "a"); _dev(head_w, "head_w")
    mode = 0 if b is None else 1
    lda, T = a.shape[1], a.shape[2]
    C = channels if channels is not None else lda
    H = head_w.shape[0]
    if head_w.shape[1] != C:
        raise ValueError("heads: head_w / channel mismatch")
    for nm, t in (("ia", ia), ("ib", ib)):
        if t is not None:
            _dev(t, nm, torch.int64)
    if b is not None:
        _dev(b, "b")
        if b.shape[1:] != a.shape[1:]:
            raise ValueError("heads: a / b shape mismatch")
    if num_pairs is None:
        num_pairs = ia.shape[0] if ia is not None else a.shape[0]
    out = torch.empty((num_pairs, H, T), dtype=torch.float32, device=a.device)
    _abi.check(_abi.lib().tspn_heads_f32(mode, _p(a), _p(b), lda, _p(ia), _p(ib), 1, _p(bias),
                                         _p(head_w), _p(head_b), H, num_pairs, C, T, _p(out), _stream()))
    return out


def heads_pairgrid(y, B, N, head_w, head_b):
    """Blocked pair stage on tracklet projections y[B*N, 2C, T] for the canonical pair table."""
    _dev(y, "y"); _dev(head_w, "head_w")
    NT, C2, T = y.shape
    C, H = C2 // 2, head_w.shape[0]
    if NT != B * N or head_w.shape[1] != C:
        raise ValueError("heads_pairgrid: shape mismatch")
    out = torch.empty((B * N * max(N - 1, 0), H, T), dtype=torch.float32, device=y.device)
    _abi.check(_abi.lib().tspn_heads_pairgrid_f32(_p(y), B, N, C, T, _p(head_w), _p(head_b), H, _p(out),
                                                  _stream()))
    return out


def heads_pairgrid_f16x3_split_bytes(C, H):
    """Bytes of scratch heads_pairgrid_f16x3 needs for C channels and H heads (0 for a C or H it refuses)."""
    return int(_abi.lib().tspn_heads_pairgrid_f16x3_split_bytes(int(C), int(H)))


def heads_pairgrid_f16x3_set_force_exact(on):
    """1 = every tile of the split-fp16 pair stage takes its fp32 chain (tests), 0 = default.  Process-wide; returns the
    previous setting."""
    return _toggle("tspn_heads_pairgrid_f16x3_set_force_exact", on)


def heads_pair_f16x3_set_diag_skip(on):
    """1 = in a diagonal tile of the split-fp16 pair stage a wave walks only the seven objects it stores (default), 0 =
    all eight as in every other tile (tspn_heads_pair_f16x3_set_diag_skip); same outputs bit for bit.  Process-wide;
    returns the previous setting."""
    return _toggle("tspn_heads_pair_f16x3_set_diag_skip", on)


def heads_pairgrid_f16x3(y, B, N, head_w, head_b, T=None, split_buf=None, out=None):
    """The canonical pair stage on split-fp16 MFMAs: y[B*N, 2C, ldt] (the first T frames of a row are used, T = ldt by
    default) -> out[B*N*(N-1), H, T].  `split_buf`: uint8 scratch of heads_pairgrid_f16x3_split_bytes(C, H) bytes."""
    _dev(y, "y"); _dev(head_w, "head_w")
    NT, C2, ldt = y.shape
    T = ldt if T is None else int(T)
    C, H = C2 // 2, head_w.shape[0]
    if NT != B * N or head_w.shape[1] != C:
        raise ValueError("heads_pairgrid_f16x3: shape mismatch")
    if split_buf is None:
        split_buf = _ws(heads_pairgrid_f16x3_split_bytes(C, H), y.device)
    if out is None:
        out = torch.empty((B * N * max(N - 1, 0), H, T), dtype=torch.float32, device=y.device)
    _abi.check(_abi.lib().tspn_heads_pairgrid_f16x3(_p(y), ldt, B, N, C, T, _p(head_w), _p(head_b), H, _p(split_buf),
                                                    split_buf.numel(), _p(out), _stream()))
    return out


def temporal_mean(x, layout_tc):
    """Mean over frames: x[R,T,D] -> [R,D] (layout_tc=True) or x[R,C,T] -> [R,C]."""
    _dev(x, "x")
    if layout_tc:
        R, T, Cd = x.shape
    else:
        R, Cd, T = x.shape
    out = torch.empty((R, Cd), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().tspn_temporal_mean_f32(_p(x), R, T, Cd, 1 if layout_tc else 0, _p(out), _stream()))
    return out


def temporal_sum(x):
    """Sum over the middle axis: x[R,T,D] -> [R,D], frames added in order (tspn_temporal_sum_f32); with R = 1 the
    column sums of a matrix (bias gradients of the training step)."""
    _dev(x, "x")
    R, T, Cd = x.shape
    out = torch.empty((R, Cd), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().tspn_temporal_sum_f32(_p(x), R, T, Cd, _p(out), _stream()))
    return out


def pair_rows(src, pairs):
    """out[P,2D] = cat(src[pairs[:,0]], src[pairs[:,1]])."""
    _dev(src, "src"); _dev(pairs, "pairs", torch.int64)
    NT, D = src.shape
    P = pairs.shape[0]
    out = torch.empty((P, 2 * D), dtype=torch.float32, device=src.device)
    _abi.check(_abi.lib().tspn_pair_rows_f32(_p(src), NT, D, _p(pairs), P, _p(out), _stream()))
    return out


def transpose_td(x):
    """[R,T,D] -> [R,D,T]."""
    _dev(x, "x")
    R, T, D = x.shape
    out = torch.empty((R, D, T), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().tspn_transpose_td_f32(_p(x), R, T, D, _p(out), _stream()))
    return out


def decode_topk(rel_logit, pairs, cls_sub, cls_obj=None, row_mul=1, num_obj=35,
                topk_per_pair=20, topk_per_seg=200, check_pairs=True):
    """Top-k triplet decode (lib/modeling/predict.py:66-106) for a batch of equal-shape segments.

    rel_logit [S,P,K] (or [P,K]); pairs int64 [S,P,2] local tracklet ids; class logits:
      * reference quirk: cls_sub = feature matrix [S,P,F] with F >= 70 (columns 0:35 subject,
        35:70 object classeme), row_mul = N-1  (predict.py:88-89 reads row (N-1)*tid);
      * per-tracklet:    cls_sub = track_cls_logits [S,N,35], row_mul = 1.
    Returns (scores [S,M], triplets int64 [S,M,3], pair_tids int64 [S,M,2]).
    """
    squeeze = rel_logit.dim() == 2
    if squeeze:
        rel_logit, pairs, cls_sub = rel_logit.unsqueeze(0), pairs.unsqueeze(0), cls_sub.unsqueeze(0)
        cls_obj = cls_obj.unsqueeze(0) if cls_obj is not None else None
    _dev(rel_logit, "rel_logit"); _dev(pairs, "pairs", torch.int64); _dev(cls_sub, "cls_sub")
    S, P, K = rel_logit.shape
    if tuple(pairs.shape) != (S, P, 2):
        raise ValueError("decode_topk: pairs must be [S,P,2]")
    if cls_sub.dim() != 3 or cls_sub.shape[0] != S:
        raise ValueError("decode_topk: class logits must be [S,rows,cols]")
    seg_rows, ld = cls_sub.shape[1], cls_sub.shape[2]
    if cls_obj is None:
        if ld >= 2 * num_obj:      # feature matrix: object classeme in columns [NO, 2NO)
            obj_ptr = cls_sub.data_ptr() + 4 * num_obj
        else:                      # per-tracklet logits: same table for both roles
            obj_ptr = cls_sub.data_ptr()
    else:
        _dev(cls_obj, "cls_obj")
        if cls_obj.shape != cls_sub.shape:
            raise ValueError("decode_topk: cls_obj shape mismatch")
        obj_ptr = cls_obj.data_ptr()
    if check_pairs and P and (int(pairs.min()) < 0 or int(pairs.max()) * row_mul >= seg_rows):
        raise IndexError("decode_topk: row_mul * tracklet id exceeds the class-logit rows")
    R = min(topk_per_pair, K)
    M = min(topk_per_seg, P * R)
    dev = rel_logit.device
    scores = torch.empty((S, M), dtype=torch.float32, device=dev)
    trip = torch.empty((S, M, 3), dtype=torch.int64, device=dev)
    tids = torch.empty((S, M, 2), dtype=torch.int64, device=dev)
    l = _abi.lib()
    ws = _ws(l.tspn_decode_topk_workspace_bytes(S, P, R), dev)
    _abi.check(l.tspn_decode_topk_f32(_p(rel_logit), _p(pairs), _p(cls_sub), ctypes.c_void_p(obj_ptr), ld,
                                      seg_rows, row_mul, S, P, K, num_obj, topk_per_pair, topk_per_seg,
                                      _p(scores), _p(trip), _p(tids), _p(ws), ws.numel(), _stream()))
    return (scores[0], trip[0], tids[0]) if squeeze else (scores, trip, tids)


def decode_spans(heads, sizes, top_k=64, nms_threshold=0.5, pre_nms=1024):
    """Temporal span proposals per pair from heads [P,3A,T] (span decode + 1-D NMS).

    Returns dict(anchor int64 [P,top_k], span int64 [P,top_k,2], span_f fp32 [P,top_k,2],
    score fp32 [P,top_k], count int64 [P])."""
    _dev(heads, "heads")
    P, H, T = heads.shape
    A = len(sizes)
    if H != 3 * A:
        raise ValueError(f"decode_spans: heads has {H} channels, expected 3*A = {3 * A}")
    dev = heads.device
    out = {"anchor": torch.empty((P, top_k), dtype=torch.int64, device=dev),
           "span": torch.empty((P, top_k, 2), dtype=torch.int64, device=dev),
           "span_f": torch.empty((P, top_k, 2), dtype=torch.float32, device=dev),
           "score": torch.empty((P, top_k), dtype=torch.float32, device=dev),
           "count": torch.empty((P,), dtype=torch.int64, device=dev)}
    sz = (ctypes.c_float * A)(*[float(v) for v in sizes])
    _abi.check(_abi.lib().tspn_decode_spans_f32(_p(heads), P, A, T, sz, top_k, float(nms_threshold), pre_nms,
                                                _p(out["anchor"]), _p(out["span"]), _p(out["span_f"]),
                                                _p(out["score"]), _p(out["count"]), _stream()))
    return out


def _span_gt(gt, P, who):
    """gt int64 [P,G,2] of the span-loss entries -> G."""
    _dev(gt, f"{who}: gt", torch.int64)
    if gt.dim() != 3 or gt.shape[2] != 2 or (P is not None and gt.shape[0] != P):
        raise ValueError(f"{who}: gt must be [P,G,2]" + ("" if P is None else f" with P = {P}") + f", got {tuple(gt.shape)}")
    return gt.shape[1]


def _anchor_sizes(sizes, who):
    sizes = [float(v) for v in sizes]
    if not sizes:
        raise ValueError(f"{who}: no anchor sizes")
    return (ctypes.c_float * len(sizes))(*sizes), len(sizes)


def span_anchor_labels(gt, sizes, num_frames, pos_iou=0.7, neg_iou=0.3):
    """Training targets of the span heads (tspn_span_anchor_labels): gt int64 [P,G,2] frames [start, end)
    per pair (end <= start = padding), `sizes` the A anchor widths -> (label int8 [P,A,T] in {1, 0, -1 = ignored},
    matched int8 [P,A,T] = the ground-truth row of the largest IoU, -1 for a pair without ground truth)."""
    who = "span_anchor_labels"
    G = _span_gt(gt, None, who)
    P, T = gt.shape[0], int(num_frames)
    sz, A = _anchor_sizes(sizes, who)
    label = torch.empty((P, A, T), dtype=torch.int8, device=gt.device)
    matched = torch.empty_like(label)
    _abi.check(_abi.lib().tspn_span_anchor_labels(_p(gt), sz, P, G, A, T, float(pos_iou), float(neg_iou), _p(label),
                                                  _p(matched), _stream()))
    return label, matched


def span_loss(heads, gt, sizes, label, matched, mask=None, beta=1.0 / 9.0):
    """Relationness and span-regression losses of one segment with their gradient (tspn_span_loss_f32 +
    tspn_span_loss_finish): heads fp32 [P,3A,T], gt int64 [P,G,2], label / matched int8 [P,A,T] from
    span_anchor_labels, mask uint8 [P,A,T] or None (0 = the loss ignores the anchor).  Returns (losses float64 [4] =
    (loss_relationness, loss_duration_proposal, n_lab, n_pos), dheads fp32 [P,3A,T] = the gradient of each loss with
    respect to its own rows, normalised).  Nothing is synchronised."""
    who = "span_loss"
    _dev(heads, f"{who}: heads")
    if heads.dim() != 3:
        raise ValueError(f"{who}: heads must be [P,3A,T], got {tuple(heads.shape)}")
    P, H, T = heads.shape
    sz, A = _anchor_sizes(sizes, who)
    if H != 3 * A:
        raise ValueError(f"{who}: heads has {H} channels, expected 3*A = {3 * A}")
    G = _span_gt(gt, P, who)
    for name, o, dt in (("label", label, torch.int8), ("matched", matched, torch.int8), ("mask", mask, torch.uint8)):
        if o is None and name == "mask":
            continue
        _dev(o, f"{who}: {name}", dt)
        if tuple(o.shape) != (P, A, T):
            raise ValueError(f"{who}: {name} must be [P,A,T] = {(P, A, T)}, got {tuple(o.shape)}")
    dev = heads.device
    partials = torch.empty((P, 4), dtype=torch.float64, device=dev)
    out = torch.empty((4,), dtype=torch.float64, device=dev)
    dheads = torch.empty_like(heads)
    lib, stream = _abi.lib(), _stream()
    _abi.check(lib.tspn_span_loss_f32(_p(heads), _p(gt), sz, _p(label), _p(matched), _p(mask), P, G, A, T, float(beta),
                                      _p(partials), _p(dheads), stream))
    _abi.check(lib.tspn_span_loss_finish(_p(partials), P, A, T, _p(out), _p(dheads), stream))
    return out, dheads


def span_anchor_sample(label, batch, positive_fraction, stream_key, key_bits=32, mask=None):
    """A balanced mini-batch of span anchors (tspn_span_anchor_sample): label int8 of any shape (the [P,A,T]
    labels of span_anchor_labels; taken flat), at most `batch` anchors selected, up to int(batch * positive_fraction) of them
    positive and negatives for the rest, in the order of the hashed keys of `stream_key` (hashrng.stream_key(seed, tag))
    shortened to `key_bits`, ties to the lower flat index.  Returns (mask uint8 of label's shape -- `mask` itself when one
    is passed -- and counts int64 [4] = (n_pos, n_neg, sel_pos, sel_neg)).  Nothing is synchronised."""
    who = "span_anchor_sample"
    if isinstance(label, torch.Tensor) and label.is_cuda and label.dtype == torch.int8:
        label = label.contiguous()
    _dev(label, f"{who}: label", torch.int8)
    batch, key_bits = int(batch), int(key_bits)
    if batch < 0 or not 0.0 <= float(positive_fraction) <= 1.0:
        raise ValueError(f"{who}: needs batch >= 0 and 0 <= positive_fraction <= 1, got {batch}, {positive_fraction}")
    want_pos = int(batch * float(positive_fraction))
    if mask is None:
        mask = torch.empty(label.shape, dtype=torch.uint8, device=label.device)
    else:
        _dev(mask, f"{who}: mask", torch.uint8)
        if mask.shape != label.shape:
            raise ValueError(f"{who}: mask must have label's shape {tuple(label.shape)}, got {tuple(mask.shape)}")
    n = label.numel()
    lib = _abi.lib()
    words = lib.tspn_span_anchor_sample_partials(n)
    if words == 0:
        raise ValueError(f"{who}: n = {n} anchors (needs < 2^31)")
    partials = torch.empty((words,), dtype=torch.int32, device=label.device)     # uint32 words; torch only carries them
    counts = torch.empty((4,), dtype=torch.int64, device=label.device)
    _abi.check(lib.tspn_span_anchor_sample(_p(label), n, int(stream_key) & 0xFFFFFFFFFFFFFFFF, key_bits, batch, want_pos,
                                           _p(partials), _p(counts), _p(mask), _stream()))
    return mask, counts


PAIR_LABEL_MERGES = {"last": 0, "or": 1}


def pair_labels(pairs, trackid, iou, insts, num_predicates, iou_thres=0.5, merge="last", max_spans=0, seg_frames=None,
                pair_off=None, track_off=None, iou_off=None, inst_off=None):
    """Training targets from ground-truth relation instances (tspn_pair_labels_f32, DESIGN.md §2 "pair labels").

    One segment: pairs int64 [P,2] (any pair table), trackid int64 [M] (< 0 proposal, >= 0 ground-truth track id), iou fp32
    [M,M], insts int64 [R,5] = (sub_tid, obj_tid, pred, begin, end).  Several segments stored back to back: iou flat, and
    int64 device offsets pair_off / track_off / iou_off / inst_off [S+1] (all four or none).  `max_spans` = G > 0 also
    wants seg_frames int64 [S,2] = (fstart, fend) on the device.  merge "last": the one-hot of the last covering instance's
    predicate (the reference's statement order); "or": every covering instance's predicate.
    Returns (labels fp32 [P,K], spans int64 [P,G,2] | None, span_count int32 [P] | None, inst_cols int32 [R,2]); a pair
    naming a track outside its segment gets span_count -1 and zero labels.  Nothing is synchronised."""
    who = "pair_labels"
    _dev(pairs, f"{who}: pairs", torch.int64); _dev(trackid, f"{who}: trackid", torch.int64)
    _dev(iou, f"{who}: iou"); _dev(insts, f"{who}: insts", torch.int64)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or trackid.dim() != 1 or insts.dim() != 2 or insts.shape[1] != 5:
        raise ValueError(f"{who}: pairs must be [P,2], trackid [M] and insts [R,5], got {tuple(pairs.shape)}, "
                         f"{tuple(trackid.shape)}, {tuple(insts.shape)}")
    if merge not in PAIR_LABEL_MERGES:
        raise ValueError(f"{who}: merge must be 'last' or 'or', got {merge!r}")
    K, G, thr = int(num_predicates), int(max_spans), float(iou_thres)
    if not 1 <= K <= 512 or not 0 <= G <= 16:
        raise ValueError(f"{who}: needs 1 <= num_predicates <= 512 and 0 <= max_spans <= 16, got {K}, {G}")
    if thr != thr or thr in (float("inf"), float("-inf")):
        raise ValueError(f"{who}: iou_thres must be finite, got {iou_thres}")
    offs = (pair_off, track_off, iou_off, inst_off)
    dev, P, M, R = pairs.device, pairs.shape[0], trackid.shape[0], insts.shape[0]
    if all(o is None for o in offs):
        S = 1
        if iou.shape != (M, M):
            raise ValueError(f"{who}: iou must be [M,M] with M = {M}, got {tuple(iou.shape)}")
    elif any(o is None for o in offs):
        raise ValueError(f"{who}: pair_off, track_off, iou_off and inst_off go together")
    else:
        for name, o in zip(("pair_off", "track_off", "iou_off", "inst_off"), offs):
            _dev(o, f"{who}: {name}", torch.int64)
        if any(o.dim() != 1 or o.shape != pair_off.shape for o in offs) or pair_off.numel() < 1:
            raise ValueError(f"{who}: the offsets must be int64 [S+1]")
        S = pair_off.numel() - 1
        if iou.dim() != 1:
            raise ValueError(f"{who}: iou of several segments must be flat, got {tuple(iou.shape)}")
    if G > 0:
        if seg_frames is None:
            raise ValueError(f"{who}: max_spans = {G} needs seg_frames [S,2]")
        _dev(seg_frames, f"{who}: seg_frames", torch.int64)
        if tuple(seg_frames.shape) != (S, 2):
            raise ValueError(f"{who}: seg_frames must be [S,2] with S = {S}, got {tuple(seg_frames.shape)}")
    labels = torch.empty((P, K), dtype=torch.float32, device=dev)
    inst_cols = torch.empty((R, 2), dtype=torch.int32, device=dev)
    spans = torch.empty((P, G, 2), dtype=torch.int64, device=dev) if G else None
    span_count = torch.empty((P,), dtype=torch.int32, device=dev) if G else None
    _abi.check(_abi.lib().tspn_pair_labels_f32(_p(pairs), _p(pair_off), _p(trackid), _p(track_off), _p(iou), _p(iou_off),
                                               _p(insts), _p(inst_off), _p(seg_frames if G else None), S, P, M, R, K, G, thr,
                                               PAIR_LABEL_MERGES[merge], _p(labels), _p(spans), _p(span_count),
                                               _p(inst_cols), _stream()))
    return labels, spans, span_count, inst_cols


def span_labels(pairs, trackid, iou, insts, num_predicates, spans, span_count, inst_cols, seg_frames, iou_thres=0.5,
                merge="last", pair_off=None, track_off=None, iou_off=None, inst_off=None):
    """A predicate label row per (pair, ground-truth span) (tspn_span_labels_f32, DESIGN.md §2 "span-pooled predicate
    training"): the operands of pair_labels (one segment, or several with the four offsets) and its outputs spans int64
    [P,G,2], span_count int32 [P], inst_cols int32 [R,2].  Row (p, g), g < min(span_count[p], G), holds the predicates of
    the instances that cover pair p and whose clipped span is spans[p, g] (merge "or": all of them, "last": the one of the
    largest r); every other row is zero.  Returns span_labels fp32 [P,G,K].  Nothing is synchronised."""
    who = "span_labels"
    _dev(pairs, f"{who}: pairs", torch.int64); _dev(trackid, f"{who}: trackid", torch.int64)
    _dev(iou, f"{who}: iou"); _dev(insts, f"{who}: insts", torch.int64)
    _dev(spans, f"{who}: spans", torch.int64); _dev(span_count, f"{who}: span_count", torch.int32)
    _dev(inst_cols, f"{who}: inst_cols", torch.int32); _dev(seg_frames, f"{who}: seg_frames", torch.int64)
    if pairs.dim() != 2 or pairs.shape[1] != 2 or trackid.dim() != 1 or insts.dim() != 2 or insts.shape[1] != 5:
        raise ValueError(f"{who}: pairs must be [P,2], trackid [M] and insts [R,5], got {tuple(pairs.shape)}, "
                         f"{tuple(trackid.shape)}, {tuple(insts.shape)}")
    if merge not in PAIR_LABEL_MERGES:
        raise ValueError(f"{who}: merge must be 'last' or 'or', got {merge!r}")
    P, M, R = pairs.shape[0], trackid.shape[0], insts.shape[0]
    if spans.dim() != 3 or spans.shape[0] != P or spans.shape[2] != 2 or span_count.shape != (P,) or inst_cols.shape != (R, 2):
        raise ValueError(f"{who}: spans must be [P,G,2], span_count [P] and inst_cols [R,2] with P = {P}, R = {R}, got "
                         f"{tuple(spans.shape)}, {tuple(span_count.shape)}, {tuple(inst_cols.shape)}")
    K, G, thr = int(num_predicates), spans.shape[1], float(iou_thres)
    if not 1 <= K <= 512 or not 1 <= G <= 16:
        raise ValueError(f"{who}: needs 1 <= num_predicates <= 512 and 1 <= G <= 16, got {K}, {G}")
    if thr != thr or thr in (float("inf"), float("-inf")):
        raise ValueError(f"{who}: iou_thres must be finite, got {iou_thres}")
    offs = (pair_off, track_off, iou_off, inst_off)
    if all(o is None for o in offs):
        S = 1
        if iou.shape != (M, M):
            raise ValueError(f"{who}: iou must be [M,M] with M = {M}, got {tuple(iou.shape)}")
    elif any(o is None for o in offs):
        raise ValueError(f"{who}: pair_off, track_off, iou_off and inst_off go together")
    else:
        for name, o in zip(("pair_off", "track_off", "iou_off", "inst_off"), offs):
            _dev(o, f"{who}: {name}", torch.int64)
        if any(o.dim() != 1 or o.shape != pair_off.shape for o in offs) or pair_off.numel() < 1:
            raise ValueError(f"{who}: the offsets must be int64 [S+1]")
        S = pair_off.numel() - 1
        if iou.dim() != 1:
            raise ValueError(f"{who}: iou of several segments must be flat, got {tuple(iou.shape)}")
    if tuple(seg_frames.shape) != (S, 2):
        raise ValueError(f"{who}: seg_frames must be [S,2] with S = {S}, got {tuple(seg_frames.shape)}")
    out = torch.empty((P, G, K), dtype=torch.float32, device=pairs.device)
    _abi.check(_abi.lib().tspn_span_labels_f32(_p(pairs), _p(pair_off), _p(trackid), _p(track_off), _p(iou), _p(iou_off),
                                               _p(insts), _p(inst_off), _p(seg_frames), S, P, M, R, K, G, thr,
                                               PAIR_LABEL_MERGES[merge], _p(spans), _p(span_count), _p(inst_cols), _p(out),
                                               _stream()))
    return out


def _span_cls_rows(who, pairs, spans, span_count):
    """(P, G) of the row operands of the span-pooled predicate training: pairs int64 [P,2], spans int64 [P,G,2],
    span_count int32 [P]."""
    _dev(pairs, f"{who}: pairs", torch.int64); _dev(spans, f"{who}: spans", torch.int64)
    _dev(span_count, f"{who}: span_count", torch.int32)
    P = pairs.shape[0]
    if tuple(pairs.shape) != (P, 2) or spans.dim() != 3 or spans.shape[0] != P or spans.shape[2] != 2 \
            or span_count.shape != (P,) or not 1 <= spans.shape[1] <= 16:
        raise ValueError(f"{who}: pairs must be [P,2], spans [P,G,2] with 1 <= G <= 16 and span_count [P], got "
                         f"{tuple(pairs.shape)}, {tuple(spans.shape)}, {tuple(span_count.shape)}")
    return P, spans.shape[1]


def span_predicate_loss(feats, pairs, spans, span_count, span_labels, cls_w, cls_b, pair_off=None, scratch=None):
    """Loss of the span-pooled predicate head on the ground-truth span rows (tspn_span_predicate_loss_f32 +
    tspn_span_predicate_loss_finish, DESIGN.md §2 "span-pooled predicate training"): feats fp32 [NT,T,D], pairs int64 [P,2]
    global tracklet ids, spans / span_count / span_labels [P,G,K] as pair_labels and span_labels return them, cls_w
    [K,2D], cls_b [K] or None, pair_off int64 [S+1] on the device (None: one segment).
    Returns (out float64 [1+S] = (loss_rel, the loss of each segment), q fp32 [P*G,K] = the sigmoid of every row, dv fp32
    [P*G,K] = d loss_rel / d v, seg_rows float64 [S], scratch uint8 = the projection scratch, free again and large enough
    for span_predicate_grad).  Nothing is synchronised."""
    who = "span_predicate_loss"
    _dev(feats, f"{who}: feats"); _dev(cls_w, f"{who}: cls_w"); _dev(span_labels, f"{who}: span_labels")
    if cls_b is not None:
        _dev(cls_b, f"{who}: cls_b")
    P, G = _span_cls_rows(who, pairs, spans, span_count)
    if feats.dim() != 3 or cls_w.dim() != 2 or cls_w.shape[1] != 2 * feats.shape[2] or \
            (cls_b is not None and cls_b.shape != (cls_w.shape[0],)):
        raise ValueError(f"{who}: feats must be [NT,T,D], cls_w [K,2D] and cls_b [K], got {tuple(feats.shape)}, "
                         f"{tuple(cls_w.shape)}")
    NT, T, D = feats.shape
    K = cls_w.shape[0]
    if tuple(span_labels.shape) != (P, G, K):
        raise ValueError(f"{who}: span_labels must be [P,G,K] = {(P, G, K)}, got {tuple(span_labels.shape)}")
    S = 1
    if pair_off is not None:
        _dev(pair_off, f"{who}: pair_off", torch.int64)
        if pair_off.dim() != 1 or pair_off.numel() < 1:
            raise ValueError(f"{who}: pair_off must be int64 [S+1]")
        S = pair_off.numel() - 1
    dev, l, stream = feats.device, _abi.lib(), _stream()
    scratch = _workspace(scratch, l.tspn_span_predicate_workspace_bytes(NT, T, D, K), dev, who)
    q = torch.empty((P * G, K), dtype=torch.float32, device=dev)
    dv = torch.empty_like(q)
    partials = torch.empty((P * G,), dtype=torch.float64, device=dev)
    seg_rows = torch.empty((S,), dtype=torch.float64, device=dev)
    out = torch.empty((1 + S,), dtype=torch.float64, device=dev)
    _abi.check(l.tspn_span_predicate_loss_f32(_p(feats), NT, T, D, _p(pairs), _p(pair_off), S, P, _p(spans), _p(span_count),
                                              _p(span_labels), G, _p(cls_w), _p(cls_b), K, _p(q), _p(dv), _p(partials),
                                              _p(seg_rows), _p(scratch), scratch.numel() * scratch.element_size(), stream))
    _abi.check(l.tspn_span_predicate_loss_finish(_p(partials), _p(seg_rows), _p(pair_off), S, P, G, K, _p(out), stream))
    return out, q, dv, seg_rows, scratch


def span_predicate_grad(dv, pairs, spans, span_count, num_tracklets, num_frames, scratch=None):
    """Gradient of the span-pooled predicate loss behind dv fp32 [P*G,K] (tspn_span_predicate_grad_f32): db fp32 [K] and
    dG fp32 [NT,T,2K], the gradient with respect to the per-frame projections (column 2k: the subject half of predicate k,
    2k+1: the object half); dW[k, h*D + c] = sum over (n, t) of dG[n, t, 2k+h] * feats[n, t, c] is a GEMM the caller runs.
    `scratch`: uint8 of at least NT*(T+1)*2K*8 bytes (span_predicate_loss returns one).  Nothing is synchronised."""
    who = "span_predicate_grad"
    _dev(dv, f"{who}: dv")
    P, G = _span_cls_rows(who, pairs, spans, span_count)
    if dv.dim() != 2 or dv.shape[0] != P * G or dv.shape[1] < 1:
        raise ValueError(f"{who}: dv must be [P*G,K] with P*G = {P * G}, got {tuple(dv.shape)}")
    NT, T, K = int(num_tracklets), int(num_frames), dv.shape[1]
    if NT < 0 or T < 1:
        raise ValueError(f"{who}: needs num_tracklets >= 0 and num_frames >= 1, got {NT}, {T}")
    dev = dv.device
    scratch = _workspace(scratch, NT * (T + 1) * 2 * K * 8, dev, who)
    db = torch.empty((K,), dtype=torch.float32, device=dev)
    dG = torch.empty((NT, T, 2 * K), dtype=torch.float32, device=dev)
    _abi.check(_abi.lib().tspn_span_predicate_grad_f32(_p(dv), _p(pairs), _p(spans), _p(span_count), NT, T, P, G, K, _p(db),
                                                       _p(dG), _p(scratch), scratch.numel() * scratch.element_size(),
                                                       _stream()))
    return db, dG


def span_match(rel_boxes, rel_range, rel_fend, rel_triplet, trk_boxes, pred_triplet, pred_pair, pred_span, iou_thr=0.5):
    """Span-bounded association of one segment (tspn_span_match_f64, DESIGN.md §2 "span match"): which relation of the
    previous segment every span-bounded prediction extends, in one call.

    rel_boxes float64 [U,2,L,4] (role 0 subject, 1 object; index f = frame f of this segment), rel_range int32 [U,2,2]
    (per role [start, end) in segment-local frames), rel_fend int32 [U], rel_triplet int64 [U,3]: the candidate relations
    in candidate order; trk_boxes float64 [N,L,4]: the segment's tracklets; pred_triplet int64 [P,3], pred_pair int32
    [P,2], pred_span int32 [P,2] = [a, e): the predictions in score order.
    Returns (match int32 [P], iou float32 [U,P,2]): match[p] = the first relation still free whose two window IoUs reach
    iou_thr, -1 for none; iou = -1 for a pair the gates refuse.  Nothing is synchronised."""
    who = "span_match"
    _dev(rel_boxes, f"{who}: rel_boxes", torch.float64); _dev(trk_boxes, f"{who}: trk_boxes", torch.float64)
    _dev(rel_range, f"{who}: rel_range", torch.int32); _dev(rel_fend, f"{who}: rel_fend", torch.int32)
    _dev(rel_triplet, f"{who}: rel_triplet", torch.int64); _dev(pred_triplet, f"{who}: pred_triplet", torch.int64)
    _dev(pred_pair, f"{who}: pred_pair", torch.int32); _dev(pred_span, f"{who}: pred_span", torch.int32)
    if rel_boxes.dim() != 4 or rel_boxes.shape[1] != 2 or rel_boxes.shape[3] != 4 or trk_boxes.dim() != 3 \
            or trk_boxes.shape[2] != 4 or trk_boxes.shape[1] != rel_boxes.shape[2]:
        raise ValueError(f"{who}: rel_boxes [U,2,L,4] and trk_boxes [N,L,4] expected, got {tuple(rel_boxes.shape)} and "
                         f"{tuple(trk_boxes.shape)}")
    U, _, L, _ = rel_boxes.shape
    N = trk_boxes.shape[0]
    if rel_range.shape != (U, 2, 2) or rel_fend.shape != (U,) or rel_triplet.shape != (U, 3):
        raise ValueError(f"{who}: rel_range must be [{U},2,2], rel_fend [{U}] and rel_triplet [{U},3], got "
                         f"{tuple(rel_range.shape)}, {tuple(rel_fend.shape)}, {tuple(rel_triplet.shape)}")
    if pred_triplet.dim() != 2 or pred_triplet.shape[1] != 3:
        raise ValueError(f"{who}: pred_triplet must be [P,3], got {tuple(pred_triplet.shape)}")
    P = pred_triplet.shape[0]
    if pred_pair.shape != (P, 2) or pred_span.shape != (P, 2):
        raise ValueError(f"{who}: pred_pair and pred_span must be [{P},2], got {tuple(pred_pair.shape)} and "
                         f"{tuple(pred_span.shape)}")
    thr = float(iou_thr)
    if thr != thr or thr in (float("inf"), float("-inf")):
        raise ValueError(f"{who}: iou_thr must be finite, got {iou_thr}")
    if U > 65536 or U * P >= 2 ** 31:
        raise ValueError(f"{who}: needs U <= 65536 and U * P < 2^31, got U = {U}, P = {P}")
    iou = torch.empty((U, P, 2), dtype=torch.float32, device=rel_boxes.device)
    match = torch.empty((P,), dtype=torch.int32, device=rel_boxes.device)
    _abi.check(_abi.lib().tspn_span_match_f64(_p(rel_boxes), _p(rel_range), _p(rel_fend), _p(rel_triplet), _p(trk_boxes),
                                              _p(pred_triplet), _p(pred_pair), _p(pred_span), U, P, N, L, thr, _p(iou),
                                              _p(match), _stream()))
    return match, iou


def _fused_desc(feats, pairs, B, N, conv_packed, conv_bias, head_w, head_b, cls_w, cls_b):
    _dev(feats, "tracklet_feats"); _dev(pairs, "pairs", torch.int64)
    _dev(conv_packed, "conv_packed", torch.int16 if conv_packed.dtype == torch.int16 else torch.float32)
    for nm, t in (("conv_bias", conv_bias), ("head_w", head_w),
                  ("head_b", head_b), ("cls_w", cls_w), ("cls_b", cls_b)):
        _dev(t, nm)
    NT, T, D = feats.shape
    if NT != B * N:
        raise ValueError(f"forward_fused: feats has {NT} tracklets, expected B*N = {B * N}")
    C = 2 * D
    H = head_w.shape[0]
    if H % 3 or head_w.shape[1] != C or head_b.shape != (H,):
        raise ValueError("forward_fused: head_w must be [3A, 2D]")
    f16x3 = conv_packed.dtype == torch.int16   # split-fp16 F(6,3) weights (pack_conv3_wino63_f16x3)
    w63 = conv_packed.dim() == 5 and not f16x3     # fragment-major Winograd F(6,3) weights (pack_conv3_wino63); else direct taps
    if f16x3 and wino63_f16x3_dims(conv_packed) != (D, 2 * C):
        raise ValueError(f"forward_fused: split-fp16 F(6,3) conv weights are for (Cin, M) = "
                         f"{wino63_f16x3_dims(conv_packed)}, expected ({D}, {2 * C})")
    if w63 and wino63_frag_dims(conv_packed) != (D, 2 * C):
        raise ValueError(f"forward_fused: Winograd F(6,3) conv weights are for (Cin, M) = "
                         f"{wino63_frag_dims(conv_packed)}, expected ({D}, {2 * C})")
    if (not w63 and not f16x3 and tuple(conv_packed.shape) != (3, D, 2 * C)) or conv_bias.shape != (C,):
        raise ValueError(f"forward_fused: conv_packed must be pack_conv3(conv.weight, split=D) = [3, D={D}, 4D={2 * C}] "
                         "or pack_conv3_wino63(conv.weight, split=D)")
    if cls_w.dim() != 2 or cls_w.shape[1] != C or cls_b.shape != (cls_w.shape[0],):
        raise ValueError("forward_fused: cls_w must be [K, 2D]")
    d = _abi.FusedDesc()
    d.B, d.N, d.T, d.D = B, N, T, D
    d.A, d.K = H // 3, cls_w.shape[0]
    d.feats, d.pairs, d.P = feats.data_ptr(), pairs.data_ptr(), pairs.shape[0]
    d.conv_packed, d.conv_bias = conv_packed.data_ptr(), conv_bias.data_ptr()
    # the packing is the choice of kernel
    d.conv_algo = _abi.CONV_WINOGRAD63_F16X3 if f16x3 else _abi.CONV_WINOGRAD63 if w63 else _abi.CONV_DIRECT
    d.head_w, d.head_b = head_w.data_ptr(), head_b.data_ptr()
    d.cls_w, d.cls_b = cls_w.data_ptr(), cls_b.data_ptr()
    return d


def fused_workspace_bytes(B, N, T, D, A, K, P, conv_algo=0):
    """Workspace of forward_fused; `conv_algo` = _abi.CONV_WINOGRAD63_F16X3 for split-fp16 F(6,3) weights (the
    other two algorithms need the same bytes)."""
    d = _abi.FusedDesc()
    d.B, d.N, d.T, d.D, d.A, d.K, d.P = B, N, T, D, A, K, P
    d.conv_algo = conv_algo
    return _abi.lib().tspn_forward_fused_workspace_bytes(ctypes.byref(d))


def forward_fused(feats, pairs, B, N, conv_packed, conv_bias, head_w, head_b, cls_w, cls_b,
                  workspace=None, out_heads=None, out_logits=None, check_pairs=True,
                  conv_events=None, canonical_pairs=False, logits_event=None, conv_weight=None, conv_check=0):
    """Whole scoring pass on tracklet tensors (tspn_forward_fused_f32).

    `conv_weight` (raw conv.weight [C,C,3]) + `conv_check` (rows): the a-posteriori accuracy guard of the F(6,3)
    conv -- that many output rows are recomputed in float64 behind the conv and the largest deviation lands in the
    device's status block (status_words()[_abi.STATUS_CONV_ERR], float bits); ignored with direct-tap weights.

    feats [B*N,T,D]; pairs int64 [P,2] global tracklet ids.
    `canonical_pairs`: `pairs` is cat_b(pair_index(N, base=b*N)) — the caller built it with
    pair_index — which lets the pair stage use the blocked kernel with computed output slots.
    `conv_events`: optional (begin, end) torch.cuda.Event pair (enable_timing=True, already
    recorded once so the handles exist) re-recorded around the dominant kernel.
    `logits_event`: optional torch.cuda.Event (already recorded once) re-recorded as soon as `rel_logits` is
    complete — the logits are computed first, so decode / PPN / gather can run on another stream behind it.
    Returns (heads [P,3A,T], rel_logits [P,K]).
    """
    d = _fused_desc(feats, pairs, B, N, conv_packed, conv_bias, head_w, head_b, cls_w, cls_b)
    P, T = pairs.shape[0], feats.shape[1]
    if check_pairs and P and (int(pairs.min()) < 0 or int(pairs.max()) >= B * N):
        raise IndexError("forward_fused: pair index out of range")
    l = _abi.lib()
    need = l.tspn_forward_fused_workspace_bytes(ctypes.byref(d))
    workspace = _workspace(workspace, need, feats.device, "forward_fused", sizes=True)
    if out_heads is None:
        out_heads = torch.empty((P, 3 * d.A, T), dtype=torch.float32, device=feats.device)
    if out_logits is None:
        out_logits = torch.empty((P, d.K), dtype=torch.float32, device=feats.device)
    d.out_heads, d.out_logits = out_heads.data_ptr(), out_logits.data_ptr()
    d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    d.canonical_pairs = 1 if canonical_pairs else 0
    if canonical_pairs and P != B * N * (N - 1):
        raise ValueError("forward_fused: canonical_pairs needs P == B*N*(N-1)")
    if conv_events is not None:
        d.ev_conv_begin, d.ev_conv_end = conv_events[0].cuda_event, conv_events[1].cuda_event
    if logits_event is not None:
        d.ev_logits_ready = logits_event.cuda_event
    if conv_weight is not None and conv_check > 0 and d.conv_algo in (_abi.CONV_WINOGRAD63, _abi.CONV_WINOGRAD63_F16X3):
        _dev(conv_weight, "conv_weight")
        if tuple(conv_weight.shape) != (2 * d.D, 2 * d.D, 3):
            raise ValueError(f"forward_fused: conv_weight must be conv.weight [C, C, 3] with C = {2 * d.D}")
        d.conv_weight, d.conv_check = conv_weight.data_ptr(), int(conv_check)
    _abi.check(l.tspn_forward_fused_f32(ctypes.byref(d), _stream()))
    return out_heads, out_logits


def conv3_spot_check(x, weight, y, split=0, bias=None, relu=False, hot=None, rows=128, ldy=None):
    """A-posteriori accuracy check of a temporal conv launch (tspn_conv3_spot_check_f32): x [B,T,Cin], raw
    weight [M,Cw,3] (`split` as in pack_conv3), y = the launch's output [B, rows of y, ldy]; `rows` output rows are
    recomputed at up to 24 columns each in float64 (`hot`: optional int64 [1] naming a sextet every row must cover, as the
    F(6,3) input transform reports it).  The largest |y - y_ref| is max-ed into the device's status
    block (status_words()[_abi.STATUS_CONV_ERR] holds its float bits)."""
    _dev(x, "x"); _dev(weight, "weight"); _dev(y, "y")
    B, T, Cin = x.shape
    M, Cw = weight.shape[0], weight.shape[1]
    if bias is not None:
        _dev(bias, "bias")
    scratch = torch.zeros(_abi.CONV_CHECK_SCRATCH_BYTES // 8, dtype=torch.int64, device=x.device)
    if hot is not None:
        _dev(hot, "hot", torch.int64)
        scratch[_abi.CONV_CHECK_HOT_OFFSET // 8:_abi.CONV_CHECK_HOT_OFFSET // 8 + 1] = hot.reshape(-1)[0:1]
    ld = int(ldy) if ldy is not None else y.shape[-1]
    _abi.check(_abi.lib().tspn_conv3_spot_check_f32(_p(x), B, T, Cin, _p(weight), M, Cw, split, _p(bias), 1 if relu else 0,
                                                    _p(y), ld, _p(scratch), rows, _stream()))


def temporal_encoder_heads(x, conv_packed, conv_bias, head_w, head_b, h_ws=None):
    """DPNHead.forward on a materialised x[P,C,T] (lib/modeling/relpn/dpn.py:69-73) -> [P,H,T]."""
    _dev(x, "x"); _dev(conv_packed, "conv_packed"); _dev(head_w, "head_w")
    P, C, T = x.shape
    if tuple(conv_packed.shape) != (3, C, C):
        raise ValueError("temporal_encoder_heads: conv_packed must be [3,C,C]")
    H = head_w.shape[0]
    if h_ws is None:
        h_ws = torch.empty_like(x)
    out = torch.empty((P, H, T), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().tspn_temporal_encoder_heads_f32(
        _p(x), P, C, T, _p(conv_packed), _p(conv_bias), _p(head_w), _p(head_b), H, _p(h_ws), _p(out),
        _stream()))
    return out


# --------------------------------------------------------------------------- #
# bf16-operand path (BASELINE config 3); semantics in csrc/tspn_bf16.hip / oracle.forward_bf16
# --------------------------------------------------------------------------- #
def cast_bf16(x):
    """fp32 -> bf16, round to nearest even (tspn_cast_bf16)."""
    _dev(x, "x")
    out = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    _abi.check(_abi.lib().tspn_cast_bf16(_p(x), x.numel(), _p(out), _stream()))
    return out


def pack_conv3_bf16(weight, split=0):
    """conv.weight [M,Cin,3] fp32 -> bf16 [3, Cp/8, Mp, 8] (split as in pack_conv3)."""
    _dev(weight, "weight")
    if weight.dim() != 3 or weight.shape[2] != 3:
        raise ValueError("pack_conv3_bf16: weight must be [M, Cin, 3]")
    M, Cin, _ = weight.shape
    Mp, Cp = (2 * M, split) if split else (M, Cin)
    out = torch.empty((3, Cp // 8, Mp, 8), dtype=torch.bfloat16, device=weight.device)
    _abi.check(_abi.lib().tspn_pack_conv3_bf16(_p(weight), M, Cin, split, _p(out), _stream()))
    return out


def pack_heads_bf16(head_w):
    """[H<=16, C] fp32 -> bf16 [C/8, 16, 8] (zero rows above H)."""
    _dev(head_w, "head_w")
    H, C = head_w.shape
    out = torch.empty((C // 8, 16, 8), dtype=torch.bfloat16, device=head_w.device)
    _abi.check(_abi.lib().tspn_pack_heads_bf16(_p(head_w), H, C, _p(out), _stream()))
    return out


def conv3_tc_bf16(x, packed, bias=None, ldm=None):
    """k=3 conv over time, bf16 operands: x bf16 [B,T,Cin] -> y fp32 channels-last [B,T,M]
    (`ldm` > M: rows padded to ldm floats, returned as [B,T,ldm] with the pad uninitialised)."""
    _dev(x, "x", torch.bfloat16); _dev(packed, "packed", torch.bfloat16)
    if bias is not None:
        _dev(bias, "bias")
    B, T, Cin = x.shape
    if packed.dim() != 4 or packed.shape[0] != 3 or packed.shape[1] * 8 != Cin or packed.shape[3] != 8:
        raise ValueError(f"conv3_tc_bf16: packed {tuple(packed.shape)} does not match Cin={Cin}")
    M = packed.shape[2]
    ldm = M if ldm is None else int(ldm)
    y = torch.empty((B, T, ldm), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().tspn_conv3_tc_bf16(_p(x), B, T, Cin, _p(packed), M, _p(bias), _p(y), ldm, _stream()))
    return y


def transpose_cast_bf16(x):
    """x fp32 [P,C,T] (DPNHead's input layout) -> bf16 channels-last [P,T,C] (tspn_transpose_cast_bf16)."""
    _dev(x, "x")
    P, C, T = x.shape
    out = torch.empty((P, T, C), dtype=torch.bfloat16, device=x.device)
    _abi.check(_abi.lib().tspn_transpose_cast_bf16(_p(x), P, C, T, _p(out), _stream()))
    return out


def temporal_encoder_heads_bf16(x, conv_packed, conv_bias, head_packed, head_b, H, y_ws=None):
    """DPNHead.forward (dpn.py:69-73) on bf16 operands: x fp32 [P,C,T] (transposed and rounded here) or bf16
    channels-last [P,T,C]; conv_packed = pack_conv3_bf16(conv.weight) (no split), head_packed =
    pack_heads_bf16(cat(relness, duration weights)); biases fp32 holding bf16 values -> heads fp32 [P,H,T]."""
    if x.dtype == torch.float32:
        x = transpose_cast_bf16(x.contiguous())
    _dev(x, "x", torch.bfloat16); _dev(conv_packed, "conv_packed", torch.bfloat16)
    _dev(head_packed, "head_packed", torch.bfloat16); _dev(head_b, "head_b")
    if conv_bias is not None:
        _dev(conv_bias, "conv_bias")
    P, T, C = x.shape
    if tuple(conv_packed.shape) != (3, C // 8, C, 8) or tuple(head_packed.shape) != (C // 8, 16, 8):
        raise ValueError(f"temporal_encoder_heads_bf16: packed weights do not match C={C}")
    if head_b.numel() != H:
        raise ValueError("temporal_encoder_heads_bf16: head_b must have H entries")
    if y_ws is None:
        y_ws = torch.empty((P, T, C), dtype=torch.float32, device=x.device)
    out = torch.empty((P, H, T), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().tspn_temporal_encoder_heads_bf16(
        _p(x), P, C, T, _p(conv_packed), _p(conv_bias), _p(head_packed), _p(head_b), H, _p(y_ws), _p(out), _stream()))
    return out


def heads_pairgrid_bf16(y, B, N, head_packed, head_b, H):
    """Pair stage on y fp32 [B*N, T, ldm >= 2C] (U | V halves, C from head_packed) -> heads fp32
    [B*N*(N-1), H, T]."""
    _dev(y, "y"); _dev(head_packed, "head_packed", torch.bfloat16); _dev(head_b, "head_b")
    BN, T, ldm = y.shape
    C = head_packed.shape[0] * 8
    if BN != B * N or ldm < 2 * C or tuple(head_packed.shape[1:]) != (16, 8) or head_b.numel() != H:
        raise ValueError("heads_pairgrid_bf16: shape mismatch")
    out = torch.empty((B * N * (N - 1), H, T), dtype=torch.float32, device=y.device)
    _abi.check(_abi.lib().tspn_heads_pairgrid_bf16(_p(y), ldm, B, N, C, T, _p(head_packed), _p(head_b),
                                                   H, _p(out), _stream()))
    return out


def temporal_mean_bf16(x):
    """bf16 [R,T,D] -> fp32 [R,D] holding bf16-rounded means."""
    _dev(x, "x", torch.bfloat16)
    R, T, D = x.shape
    out = torch.empty((R, D), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().tspn_temporal_mean_bf16(_p(x), R, T, D, _p(out), _stream()))
    return out


def fused_bf16_workspace_bytes(B, N, T, D, A, K, P, canonical_pairs=True):
    d = _abi.FusedBf16Desc()
    d.B, d.N, d.T, d.D, d.A, d.K, d.P = B, N, T, D, A, K, P
    l = _abi.lib()
    return (l.tspn_forward_fused_bf16_workspace_bytes if canonical_pairs
            else l.tspn_forward_fused_bf16_pairs_workspace_bytes)(ctypes.byref(d))


def _unsupported(fn):
    """The operand checks of the pair-list entries: what `_dev` refuses (dtype, device, layout) is reported the way the
    library reports an operand it cannot take, TspnError(TSPN_EUNSUPPORTED)."""
    try:
        return fn()
    except _abi.TspnError:
        raise
    except (TypeError, ValueError, RuntimeError) as exc:
        raise _abi.TspnError(_abi.TSPN_EUNSUPPORTED, str(exc)) from exc


def _check_pair_table(pairs, B, N, who):
    """Host-synchronising test of a [P,2] table of global ids: every id in [0, B*N), both ids of a row in one video."""
    if pairs.numel() == 0:
        return
    lo, hi = int(pairs.min()), int(pairs.max())
    if lo < 0 or hi >= B * N:
        raise IndexError(f"{who}: pair index out of range [0, {B * N}) (min {lo}, max {hi})")
    if B > 1 and bool((torch.div(pairs[:, 0], N, rounding_mode="floor")
                       != torch.div(pairs[:, 1], N, rounding_mode="floor")).any()):
        raise IndexError(f"{who}: a pair joins tracklets of two different videos")


def pair_plan(pairs, B, N):
    """The plan of the bf16 pair-list stage (tspn_pair_plan_i32) for pairs int64 [P,2] (global ids, video = id // N):
    dict of int32 tensors `s_list` / `o_list` [B,Np] (the distinct subjects / objects of each video, local ids,
    ascending; Np = N rounded up to 16), `counts` [B,2], `head` [B,Np,Np] (first row of the chain of rows whose pair is
    (s_list[b][i], o_list[b][j]), -1 for none) and `next` [P].  Rows with an id out of range or ids in two videos are on
    no chain.  The order of a chain differs from run to run; the set of rows on it does not."""
    _unsupported(lambda: _dev(pairs, "pairs", torch.int64))
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise _abi.TspnError(_abi.TSPN_EUNSUPPORTED, "pair_plan: pairs must be [P,2]")
    B, N, P = int(B), int(N), pairs.shape[0]
    Np = (N + 15) // 16 * 16
    i32 = dict(dtype=torch.int32, device=pairs.device)
    plan = {"s_list": torch.empty((B, Np), **i32), "o_list": torch.empty((B, Np), **i32),
            "counts": torch.empty((B, 2), **i32), "head": torch.empty((B, Np, Np), **i32), "next": torch.empty((P,), **i32)}
    rank_ws = torch.empty((B, 2, max(N, 1)), **i32)
    _abi.check(_abi.lib().tspn_pair_plan_i32(_p(pairs), P, B, N, _p(plan["s_list"]), _p(plan["o_list"]), _p(plan["counts"]),
                                             _p(plan["head"]), _p(plan["next"]), _p(rank_ws), _stream()))
    return plan


def heads_pairlist_bf16(y, pairs, B, N, head_packed, head_b, H, check_pairs=True, out=None):
    """Pair stage on y fp32 [B*N, T, ldm >= 2C] (U | V halves, C from head_packed) for ANY pair table: pairs int64 [P,2]
    of global ids, any order, any subset, repeated rows and (s, s) rows allowed -> heads fp32 [P, H, T]; a row equals,
    bit for bit, heads_pairgrid_bf16's row of the same (s, o).  `check_pairs` = the host-synchronising range and
    same-video test (IndexError); without it a row that fails the test is skipped and its row of `out` left unwritten.
    `out`: a contiguous fp32 [P, H, T] to write into."""
    def operands():
        _dev(y, "y"); _dev(pairs, "pairs", torch.int64)
        _dev(head_packed, "head_packed", torch.bfloat16); _dev(head_b, "head_b")
        if out is not None:
            _dev(out, "out")
    _unsupported(operands)
    if y.dim() != 3 or pairs.dim() != 2 or pairs.shape[1] != 2 or head_packed.dim() != 3:
        raise ValueError("heads_pairlist_bf16: y must be [B*N,T,ldm], pairs [P,2], head_packed [C/8,16,8]")
    BN, T, ldm = y.shape
    C = head_packed.shape[0] * 8
    P = pairs.shape[0]
    if BN != B * N or tuple(head_packed.shape[1:]) != (16, 8) or head_b.numel() != H:
        raise ValueError("heads_pairlist_bf16: shape mismatch")
    if check_pairs:
        _check_pair_table(pairs, B, N, "heads_pairlist_bf16")
    if out is None:
        out = torch.empty((P, H, T), dtype=torch.float32, device=y.device)
    elif tuple(out.shape) != (P, H, T):
        raise ValueError("heads_pairlist_bf16: out shape mismatch")
    l = _abi.lib()
    need = l.tspn_heads_pairlist_bf16_workspace_bytes(B, N, P)
    ws = _ws(need, y.device)
    _abi.check(l.tspn_heads_pairlist_bf16(_p(y), ldm, B, N, C, T, _p(pairs), P, _p(head_packed), _p(head_b), H, _p(out),
                                          _p(ws), ws.numel(), _stream()))
    return out


def forward_fused_bf16(feats, pairs, B, N, conv_packed, conv_bias, head_packed, head_b, cls_w, cls_b,
                       workspace=None, conv_events=None, logits_event=None, out_heads=None, out_logits=None,
                       canonical_pairs=True, check_pairs=True):
    """Whole scoring pass, bf16 operands: tspn_forward_fused_bf16 on the canonical pair table (the default), or, with
    `canonical_pairs=False`, tspn_forward_fused_bf16_pairs on any [P,2] table of global ids (pair-list stage; its
    workspace is fused_bf16_workspace_bytes(..., canonical_pairs=False)).  `check_pairs` (pair tables only) = the
    host-synchronising range and same-video test of heads_pairlist_bf16 (IndexError).

    feats bf16 [B*N,T,D]; conv_packed = pack_conv3_bf16(conv.weight, split=D); head_packed =
    pack_heads_bf16([3A,C]); cls_w fp32 [K,C] holding bf16-rounded values.
    Returns (heads fp32 [P,3A,T], rel_logits fp32 [P,K])."""
    _dev(feats, "feats", torch.bfloat16); _dev(pairs, "pairs", torch.int64)
    _dev(conv_packed, "conv_packed", torch.bfloat16); _dev(conv_bias, "conv_bias")
    _dev(head_packed, "head_packed", torch.bfloat16); _dev(head_b, "head_b")
    _dev(cls_w, "cls_w"); _dev(cls_b, "cls_b")
    BN, T, D = feats.shape
    C = 2 * D
    if BN != B * N:
        raise ValueError("forward_fused_bf16: feats rows != B*N")
    if tuple(conv_packed.shape) != (3, D // 8, 2 * C, 8):
        raise ValueError(f"forward_fused_bf16: conv_packed {tuple(conv_packed.shape)} != {(3, D // 8, 2 * C, 8)}")
    if tuple(head_packed.shape) != (C // 8, 16, 8) or head_b.numel() % 3:
        raise ValueError("forward_fused_bf16: head weights do not match C")
    A, K = head_b.numel() // 3, cls_w.shape[0]
    if tuple(cls_w.shape) != (K, C) or conv_bias.numel() != C or cls_b.numel() != K:
        raise ValueError("forward_fused_bf16: classifier / bias shapes do not match")
    P = pairs.shape[0]
    if canonical_pairs:
        if tuple(pairs.shape) != (B * N * (N - 1), 2):
            raise ValueError("forward_fused_bf16: needs the canonical pair table [B*N*(N-1), 2]")
    else:
        if pairs.dim() != 2 or pairs.shape[1] != 2:
            raise ValueError("forward_fused_bf16: pairs must be [P,2]")
        if check_pairs:
            _check_pair_table(pairs, B, N, "forward_fused_bf16")
    d = _abi.FusedBf16Desc()
    d.B, d.N, d.T, d.D, d.A, d.K, d.P = B, N, T, D, A, K, P
    d.feats, d.pairs = feats.data_ptr(), pairs.data_ptr()
    d.conv_packed, d.conv_bias = conv_packed.data_ptr(), conv_bias.data_ptr()
    d.head_packed, d.head_b = head_packed.data_ptr(), head_b.data_ptr()
    d.cls_w, d.cls_b = cls_w.data_ptr(), cls_b.data_ptr()
    l = _abi.lib()
    need = (l.tspn_forward_fused_bf16_workspace_bytes if canonical_pairs
            else l.tspn_forward_fused_bf16_pairs_workspace_bytes)(ctypes.byref(d))
    workspace = _workspace(workspace, need, feats.device, "forward_fused_bf16")
    if out_heads is None:
        out_heads = torch.empty((P, 3 * A, T), dtype=torch.float32, device=feats.device)
    elif tuple(out_heads.shape) != (P, 3 * A, T):
        raise ValueError("forward_fused_bf16: out_heads shape mismatch")
    if out_logits is None:
        out_logits = torch.empty((P, K), dtype=torch.float32, device=feats.device)
    elif tuple(out_logits.shape) != (P, K):
        raise ValueError("forward_fused_bf16: out_logits shape mismatch")
    _dev(out_heads, "out_heads"); _dev(out_logits, "out_logits")
    d.out_heads, d.out_logits = out_heads.data_ptr(), out_logits.data_ptr()
    d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    if conv_events is not None:
        d.ev_conv_begin, d.ev_conv_end = conv_events[0].cuda_event, conv_events[1].cuda_event
    if logits_event is not None:
        d.ev_logits_ready = logits_event.cuda_event
    _abi.check((l.tspn_forward_fused_bf16 if canonical_pairs else l.tspn_forward_fused_bf16_pairs)(ctypes.byref(d), _stream()))
    return out_heads, out_logits


def _span_rows(who, NT, pairs, spans, classifier_ok=True):
    """P of span_predicate / span_predicate_bf16: pairs and spans are [P,2] (one refusal with the fp32 wrapper's
    classifier shape), and the host-synchronising range test of the tracklet ids."""
    P = pairs.shape[0]
    if not classifier_ok or tuple(pairs.shape) != (P, 2) or tuple(spans.shape) != (P, 2):
        raise ValueError(f"{who}: shape mismatch")
    if P and (int(pairs.min()) < 0 or int(pairs.max()) >= NT):
        raise IndexError(f"{who}: pair index out of range")
    return P


def span_predicate(feats, pairs, spans, cls_w, cls_b):
    """Span-restricted RelOIPool + predicate head (tspn_span_predicate_f32): feats [NT,T,D], pairs [P,2]
    global tracklet ids, spans int64 [P,2] frames [start,end) -> sigmoid logits [P,K]."""
    _dev(feats, "feats"); _dev(pairs, "pairs", torch.int64); _dev(spans, "spans", torch.int64)
    _dev(cls_w, "cls_w")
    if cls_b is not None:
        _dev(cls_b, "cls_b")
    NT, T, D = feats.shape
    K = cls_w.shape[0]
    P = _span_rows("span_predicate", NT, pairs, spans, tuple(cls_w.shape) == (K, 2 * D))
    l = _abi.lib()
    ws = _ws(l.tspn_span_predicate_workspace_bytes(NT, T, D, K), feats.device)
    out = torch.empty((P, K), dtype=torch.float32, device=feats.device)
    _abi.check(l.tspn_span_predicate_f32(_p(feats), NT, T, D, _p(pairs), _p(spans), P, _p(cls_w), _p(cls_b), K,
                                         _p(out), _p(ws), ws.numel(), _stream()))
    return out


def _decode_span_relations(who, entry, ws_query, classifier, classifier_last, feats, pairs, spans, span_scores,
                           span_counts, cls, cls_b, cls_logits, topk_per_span, topk_per_seg, check_pairs, out):
    """decode_span_relations and decode_span_relations_bf16 behind their `_dev` lines: one body.  `entry`, `ws_query`: the
    names of the C entry and of its workspace query; `classifier(D)` checks `cls` / `cls_b` and returns K, after the spans'
    checks where `classifier_last` (the fp32 wrapper), before them otherwise."""
    if pairs.dim() != 3 or pairs.shape[2] != 2 or cls_logits.dim() != 3 or cls_logits.shape[0] != pairs.shape[0]:
        raise ValueError(f"{who}: pairs must be [S,P,2] and cls_logits [S,N,num_obj]")
    S, P, _ = pairs.shape
    N, NO = cls_logits.shape[1], cls_logits.shape[2]
    if feats.dim() == 4:
        feats = feats.view(-1, feats.shape[2], feats.shape[3])
    if feats.dim() != 3 or feats.shape[0] != S * N:
        raise ValueError(f"{who}: feats must hold S*N = {S * N} tracklets [S*N,T,D], got {tuple(feats.shape)}")
    T, D = feats.shape[1], feats.shape[2]
    if not classifier_last:
        K = classifier(D)
    if spans.dim() < 3 or spans.shape[-1] != 2:
        raise ValueError(f"{who}: spans must be [S*P,J,2]")
    J = spans.shape[-2]
    if spans.numel() != S * P * J * 2 or span_scores.numel() != S * P * J or span_counts.numel() != S * P \
            or (span_scores.numel() and span_scores.shape[-1] != J):
        raise ValueError(f"{who}: spans [S*P,J,2], span_scores [S*P,J] and span_counts [S*P] expected for "
                         f"S*P = {S * P}, J = {J}")
    if classifier_last:
        K = classifier(D)
    if check_pairs and S * P and (int(pairs.min()) < 0 or int(pairs.max()) >= N):
        raise IndexError(f"{who}: tracklet id outside the segment")
    R = min(int(topk_per_span), K)
    Mc = min(int(topk_per_seg), P * J * R)
    dev = feats.device
    shapes = (((S, Mc), torch.float32), ((S, Mc, 3), torch.int64), ((S, Mc, 2), torch.int64), ((S, Mc, 2), torch.int64),
              ((S, Mc), torch.int64), ((S,), torch.int64))
    if out is None:
        out = tuple(torch.empty(sh, dtype=dt, device=dev) for sh, dt in shapes)
        if S * P == 0:
            out[5].zero_()                       # nothing is launched
    else:
        if len(out) != 6:
            raise ValueError(f"{who}: out must be the six result tensors")
        for t, (sh, dt), name in zip(out, shapes, ("scores", "triplets", "pair_tids", "spans", "span_rank", "valid")):
            if tuple(_dev(t, "out." + name, dt).shape) != sh:
                raise ValueError(f"{who}: out.{name} must be {sh}")
    l = _abi.lib()
    ws = _ws(getattr(l, ws_query)(S, N, T, D, P, J, K, int(topk_per_span)), dev)
    _abi.check(getattr(l, entry)(_p(feats), S, N, T, D, _p(pairs), P, _p(spans), _p(span_scores), _p(span_counts), J,
                                 _p(cls), _p(cls_b), K, _p(cls_logits), NO, int(topk_per_span), int(topk_per_seg),
                                 *[_p(t) for t in out], _p(ws), ws.numel(), _stream()))
    return tuple(out)


def decode_span_relations(feats, pairs, spans, span_scores, span_counts, cls_w, cls_b, cls_logits, topk_per_span=20,
                          topk_per_seg=200, check_pairs=True, out=None):
    """Relations with their temporal spans for S equal-shape segments (tspn_decode_span_relations_f32).

    feats [S,N,T,D] (or [S*N,T,D]); pairs int64 [S,P,2] segment-local tracklet ids; spans int64 [S*P,J,2],
    span_scores [S*P,J], span_counts int64 [S*P]: `decode_spans(top_k=J)` of the S*P pairs (leading dims [S,P] are taken
    too); cls_w [K,2D], cls_b [K] or None; cls_logits [S,N,num_obj].  A candidate (pair, span j < count, predicate k)
    scores span_predicate(pair, span)[k] * span_score: per span the `topk_per_span` best k, per segment the
    `topk_per_seg` best candidates.
    Returns (scores [S,Mc], triplets int64 [S,Mc,3], pair_tids int64 [S,Mc,2], spans int64 [S,Mc,2], span_rank int64
    [S,Mc], valid int64 [S]) with Mc = min(topk_per_seg, P*J*min(topk_per_span, K)); segment s has valid[s] <= Mc real
    rows, the rest are not written.  `out`: those six tensors, preallocated."""
    _dev(feats, "feats"); _dev(pairs, "pairs", torch.int64); _dev(spans, "spans", torch.int64)
    _dev(span_scores, "span_scores"); _dev(span_counts, "span_counts", torch.int64)
    _dev(cls_w, "cls_w"); _dev(cls_logits, "cls_logits")
    if cls_b is not None:
        _dev(cls_b, "cls_b")

    def classifier(D):
        K = cls_w.shape[0]
        if tuple(cls_w.shape) != (K, 2 * D) or (cls_b is not None and tuple(cls_b.shape) != (K,)):
            raise ValueError("decode_span_relations: cls_w must be [K,2D] and cls_b [K]")
        return K
    return _decode_span_relations("decode_span_relations", "tspn_decode_span_relations_f32",
                                  "tspn_decode_span_relations_workspace_bytes", classifier, True, feats, pairs, spans,
                                  span_scores, span_counts, cls_w, cls_b, cls_logits, topk_per_span, topk_per_seg,
                                  check_pairs, out)


def pack_span_cls_bf16(cls_w):
    """Classifier weight fp32 [K, 2D] (D % 16 == 0) -> the packed bf16 image of the bf16 span entries
    (tspn_pack_span_cls_bf16): [ceil(K/16), 2D/32, 64, 8], fragment-major, rounded to nearest even, rows past K zero."""
    _dev(cls_w, "cls_w")
    if cls_w.dim() != 2 or cls_w.shape[1] % 2:
        raise ValueError("pack_span_cls_bf16: cls_w must be [K, 2D]")
    K, D = cls_w.shape[0], cls_w.shape[1] // 2
    if K < 1 or D < 1 or D % 16:
        raise ValueError(f"the bf16 path needs D % 16 == 0 (D={D})")
    packed = torch.empty(((K + 15) // 16, 2 * D // 32, 64, 8), dtype=torch.bfloat16, device=cls_w.device)
    _abi.check(_abi.lib().tspn_pack_span_cls_bf16(_p(cls_w), K, D, _p(packed), _stream()))
    return packed


def _span_cls_packed(cls_packed, cls_b, K, D, who):
    _dev(cls_packed, "cls_packed", torch.bfloat16)
    if cls_b is not None:
        _dev(cls_b, "cls_b")
    K = int(K)
    if D % 16:
        raise ValueError(f"the bf16 path needs D % 16 == 0 (D={D})")
    if K < 1 or tuple(cls_packed.shape) != ((K + 15) // 16, 2 * D // 32, 64, 8) or (cls_b is not None and tuple(cls_b.shape) != (K,)):
        raise ValueError(f"{who}: cls_packed must be pack_span_cls_bf16 of a [K={K}, 2D={2 * D}] weight and cls_b [K]")
    return K


def span_predicate_bf16(feats, pairs, spans, cls_packed, cls_b, K, out=None, workspace=None):
    """Span-restricted RelOIPool + predicate head on a bf16 segment (tspn_span_predicate_bf16): feats
    bf16 [NT,T,D] (D % 16 == 0), pairs int64 [P,2] global tracklet ids (any table: repeated rows, (i, i)), spans int64
    [P,2] frames [start,end), cls_packed = pack_span_cls_bf16(cls_w [K,2D]), cls_b fp32 [K] or None (rounded to bf16 by
    the kernel) -> sigmoid logits fp32 [P,K].  `out`: a contiguous fp32 [P,K] to write into; `workspace`: a uint8 tensor
    of at least tspn_span_predicate_bf16_workspace_bytes."""
    _dev(feats, "feats", torch.bfloat16); _dev(pairs, "pairs", torch.int64); _dev(spans, "spans", torch.int64)
    if feats.dim() != 3:
        raise ValueError("span_predicate_bf16: feats must be [NT,T,D]")
    NT, T, D = feats.shape
    K = _span_cls_packed(cls_packed, cls_b, K, D, "span_predicate_bf16")
    P = _span_rows("span_predicate_bf16", NT, pairs, spans)
    if out is None:
        out = torch.empty((P, K), dtype=torch.float32, device=feats.device)
    elif tuple(_dev(out, "out").shape) != (P, K):
        raise ValueError("span_predicate_bf16: out shape mismatch")
    l = _abi.lib()
    need = l.tspn_span_predicate_bf16_workspace_bytes(NT, T, D, K, P)
    workspace = _workspace(workspace, need, feats.device, "span_predicate_bf16")
    _abi.check(l.tspn_span_predicate_bf16(_p(feats), NT, T, D, _p(pairs), _p(spans), P, _p(cls_packed), _p(cls_b), K,
                                          _p(out), _p(workspace), workspace.numel() * workspace.element_size(), _stream()))
    return out


def decode_span_relations_bf16(feats, pairs, spans, span_scores, span_counts, cls_packed, cls_b, K, cls_logits,
                               topk_per_span=20, topk_per_seg=200, check_pairs=True, out=None):
    """decode_span_relations for S equal-shape bf16 segments (tspn_decode_span_relations_bf16): feats bf16 [S,N,T,D] (or
    [S*N,T,D]), cls_packed = pack_span_cls_bf16(cls_w [K,2D]), cls_b fp32 [K] or None; every other argument and the six
    results as decode_span_relations.  A candidate's predicate value is span_predicate_bf16's for that (pair, span) row,
    bit for bit."""
    who = "decode_span_relations_bf16"
    _dev(feats, "feats", torch.bfloat16); _dev(pairs, "pairs", torch.int64); _dev(spans, "spans", torch.int64)
    _dev(span_scores, "span_scores"); _dev(span_counts, "span_counts", torch.int64); _dev(cls_logits, "cls_logits")
    return _decode_span_relations(who, "tspn_decode_span_relations_bf16",
                                  "tspn_decode_span_relations_bf16_workspace_bytes",
                                  lambda D: _span_cls_packed(cls_packed, cls_b, K, D, who), False, feats, pairs, spans,
                                  span_scores, span_counts, cls_packed, cls_b, cls_logits, topk_per_span, topk_per_seg,
                                  check_pairs, out)


# --------------------------------------------------------------------------- #
# f4 (first slice): RoI feature head operators (csrc/tspn_roi.hip)
# --------------------------------------------------------------------------- #
def pack_conv2d(weight):
    """nn.Conv2d weight [Cout,Cin,KH,KW] -> [KH*KW, Cin, Cout] (tspn_pack_conv2d_f32)."""
    _dev(weight, "conv2d weight")
    if weight.dim() != 4:
        raise ValueError("pack_conv2d: weight must be [Cout,Cin,KH,KW]")
    Cout, Cin, KH, KW = weight.shape
    packed = torch.empty((KH * KW, Cin, Cout), dtype=torch.float32, device=weight.device)
    _abi.check(_abi.lib().tspn_pack_conv2d_f32(_p(weight), Cout, Cin, KH, KW, _p(packed), _stream()))
    return packed


def pack_conv2d_frag(weight):
    """nn.Conv2d weight [Cout,Cin,KH,KW] -> fragment-major [Cout/32, KH*KW, Cin/16, 64, 8]
    (tspn_pack_conv2d_frag_f32; the registers-direct kernel).  Needs Cout % 32 == 0, Cin % 16 == 0."""
    _dev(weight, "conv2d weight")
    if weight.dim() != 4:
        raise ValueError("pack_conv2d_frag: weight must be [Cout,Cin,KH,KW]")
    Cout, Cin, KH, KW = weight.shape
    if Cout % 32 or Cin % 16:
        raise ValueError(f"pack_conv2d_frag: needs Cout % 32 == 0 and Cin % 16 == 0 (Cout={Cout}, Cin={Cin})")
    frag = torch.empty((Cout // 32, KH * KW, Cin // 16, 64, 8), dtype=torch.float32, device=weight.device)
    _abi.check(_abi.lib().tspn_pack_conv2d_frag_f32(_p(weight), Cout, Cin, KH, KW, _p(frag), _stream()))
    return frag


def _bias_residual(who, bias, residual, out_shape, dtype):
    """The optional epilogue operands of conv2d_nhwc / conv2d_nhwc_bf16: bias fp32 [Cout], residual `dtype` of the output's
    shape."""
    if bias is not None:
        _dev(bias, "bias")
        if bias.shape != (out_shape[3],):
            raise ValueError(f"{who}: bias shape mismatch")
    if residual is not None:
        _dev(residual, "residual", dtype)
        if tuple(residual.shape) != tuple(out_shape):
            raise ValueError(f"{who}: residual shape mismatch")


def conv2d_nhwc(x, packed, kernel_size, stride=1, padding=0, bias=None, residual=None, relu=False):
    """act(conv2d(x) + bias + residual) on channels-last tensors: x [NB,H,W,Cin] -> [NB,OH,OW,Cout];
    `packed` = pack_conv2d(weight) or pack_conv2d_frag(weight) (5-D: fast kernel), kernel_size = (KH, KW)."""
    _dev(x, "x"); _dev(packed, "packed")
    NB, H, W, Cin = x.shape
    KH, KW = kernel_size
    frag = packed.dim() == 5
    if frag:
        if tuple(packed.shape[1:]) != (KH * KW, Cin // 16, 64, 8) or Cin % 16:
            raise ValueError(f"conv2d_nhwc: fragment-major weights {tuple(packed.shape)} do not match "
                             f"taps={KH * KW}, Cin={Cin}")
        Cout = packed.shape[0] * 32
    else:
        if packed.dim() != 3 or packed.shape[0] != KH * KW or packed.shape[1] != Cin:
            raise ValueError(f"conv2d_nhwc: packed weights {tuple(packed.shape)} do not match taps={KH * KW}, Cin={Cin}")
        Cout = packed.shape[2]
    OH, OW = _out_hw("conv2d_nhwc", H, W, KH, KW, stride, padding)
    _bias_residual("conv2d_nhwc", bias, residual, (NB, OH, OW, Cout), torch.float32)
    out = torch.empty((NB, OH, OW, Cout), dtype=torch.float32, device=x.device)
    fn = _abi.lib().tspn_conv2d_nhwc_frag_f32 if frag else _abi.lib().tspn_conv2d_nhwc_f32
    _abi.check(fn(_p(x), NB, H, W, Cin, _p(packed), Cout, KH, KW, stride, padding,
                  _p(bias), _p(residual), 1 if relu else 0, _p(out), _stream()))
    return out


def roi_align_nhwc(feat, rois, output_size, spatial_scale, sampling_ratio=0, aligned=True, out_bf16=False,
                   bin_stride=1):
    """detectron2 ROIAlign on a channels-last map: feat [NF,H,W,C], rois [R,5] = (map index, x1, y1, x2, y2)
    -> [R,P,P,C]; `out_bf16`: the fp32 result rounded once to bf16.  A bf16 map is read as it is
    (interpolation in fp32) and always gives bf16.  `bin_stride` = bs: only the bins (bs i, bs j) -> [R,OP,OP,C],
    OP = ceil(P / bs)."""
    bf16_in = isinstance(feat, torch.Tensor) and feat.dtype == torch.bfloat16
    _dev(feat, "feat", torch.bfloat16 if bf16_in else torch.float32); _dev(rois, "rois")
    out_bf16 = out_bf16 or bf16_in
    NF, H, W, C = feat.shape
    if rois.dim() != 2 or rois.shape[1] != 5:
        raise ValueError("roi_align_nhwc: rois must be [R,5]")
    R, P, bs = rois.shape[0], int(output_size), int(bin_stride)
    if bs < 1:
        raise ValueError("roi_align_nhwc: bin_stride must be >= 1")
    OP = (P + bs - 1) // bs
    out = torch.empty((R, OP, OP, C), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=feat.device)
    fn = _abi.lib().tspn_roi_align_nhwc_bf16 if bf16_in else (
        _abi.lib().tspn_roi_align_nhwc_f32_bf16out if out_bf16 else _abi.lib().tspn_roi_align_nhwc_f32)
    _abi.check(fn(_p(feat), NF, H, W, C, _p(rois), R, P, float(spatial_scale),
                  int(sampling_ratio), 1 if aligned else 0, bs, _p(out), _stream()))
    return out


def _frag_shape_bf16(cout, cin, taps):
    """Shape of pack_conv2d_frag_bf16's result for a [cout, cin, KH, KW] weight with KH * KW = taps."""
    return (cout // 32, cin // 64, taps, 4, 64, 8)


def _out_bf16(out, shape, device, who):
    """`out` checked to be a bf16 device tensor of `shape`, or a new one when None."""
    if out is None:
        return torch.empty(shape, dtype=torch.bfloat16, device=device)
    _dev(out, "out", torch.bfloat16)
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"{who}: out must be {tuple(shape)}, got {tuple(out.shape)}")
    return out


def pack_conv2d_frag_bf16(weight):
    """fp32 nn.Conv2d weight [Cout,Cin,KH,KW] -> bf16 fragment-major [Cout/32, Cin/64, KH*KW, 4, 64, 8]
    (tspn_pack_conv2d_frag_bf16; rounded once, to nearest even).  Needs Cout % 32 == 0, Cin % 64 == 0."""
    _dev(weight, "conv2d weight")
    if weight.dim() != 4:
        raise ValueError("pack_conv2d_frag_bf16: weight must be [Cout,Cin,KH,KW]")
    Cout, Cin, KH, KW = weight.shape
    if Cout % 32 or Cin % 64:
        raise ValueError(f"pack_conv2d_frag_bf16: needs Cout % 32 == 0 and Cin % 64 == 0 (Cout={Cout}, Cin={Cin})")
    frag = torch.empty(_frag_shape_bf16(Cout, Cin, KH * KW), dtype=torch.bfloat16, device=weight.device)
    _abi.check(_abi.lib().tspn_pack_conv2d_frag_bf16(_p(weight), Cout, Cin, KH, KW, _p(frag), _stream()))
    return frag


def conv2d_nhwc_bf16(x, frag, kernel_size, stride=1, padding=0, bias=None, residual=None, relu=False):
    """bf16-operand conv2d on channels-last tensors (tspn_conv2d_nhwc_bf16): x bf16 [NB,H,W,Cin], frag =
    pack_conv2d_frag_bf16(weight), bias fp32 [Cout], residual bf16 -> bf16 [NB,OH,OW,Cout]
    = bf16(act(fp32 sum of exact products + bias + residual))."""
    _dev(x, "x", torch.bfloat16); _dev(frag, "frag", torch.bfloat16)
    NB, H, W, Cin = x.shape
    KH, KW = kernel_size
    if frag.dim() != 6 or tuple(frag.shape[1:]) != _frag_shape_bf16(32, Cin, KH * KW)[1:] or Cin % 64:
        raise ValueError(f"conv2d_nhwc_bf16: weights {tuple(frag.shape)} do not match taps={KH * KW}, Cin={Cin}")
    Cout = frag.shape[0] * 32
    OH, OW = _out_hw("conv2d_nhwc_bf16", H, W, KH, KW, stride, padding)
    _bias_residual("conv2d_nhwc_bf16", bias, residual, (NB, OH, OW, Cout), torch.bfloat16)
    out = torch.empty((NB, OH, OW, Cout), dtype=torch.bfloat16, device=x.device)
    _abi.check(_abi.lib().tspn_conv2d_nhwc_bf16(_p(x), NB, H, W, Cin, _p(frag), Cout, KH, KW, stride, padding,
                                                _p(bias), _p(residual), 1 if relu else 0, _p(out), _stream()))
    return out


def max_pool_nhwc(x, kernel_size=3, stride=2, padding=1, out_bf16=False):
    """max_pool2d on a channels-last fp32 map [NB,H,W,C] -> [NB,OH,OW,C] (fp32, or bf16 rounded once)."""
    _dev(x, "x")
    NB, H, W, C = x.shape
    OH, OW = _out_hw("max_pool_nhwc", H, W, kernel_size, kernel_size, stride, padding)
    out = torch.empty((NB, OH, OW, C), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=x.device)
    _abi.check(_abi.lib().tspn_max_pool_nhwc_f32(_p(x), NB, H, W, C, kernel_size, stride, padding, _p(out),
                                                 1 if out_bf16 else 0, _stream()))
    return out


def _block_operands(x, frags, biases, residual=None):
    """The operand check of the three bottleneck_block*_bf16 wrappers: x (and a residual) bf16, frag1 .. frag3 (and frags)
    bf16, their biases fp32, all contiguous device tensors."""
    _dev(x, "x", torch.bfloat16)
    if residual is not None:
        _dev(residual, "residual", torch.bfloat16)
    for nm, t in zip(("frag1", "frag2", "frag3", "frags"), frags):
        _dev(t, nm, torch.bfloat16)
    for nm, t in zip(("bias1", "bias2", "bias3", "biass"), biases):
        _dev(t, nm)


def _block_frags_match(frags, CIN, CM):
    """frag1 .. frag3 (and frags) are pack_conv2d_frag_bf16 of [CM,CIN,1,1] / [CM,CM,3,3] / [4CM,CM,1,1] (/ [4CM,CIN,1,1])."""
    want = (_frag_shape_bf16(CM, CIN, 1), _frag_shape_bf16(CM, CM, 9), _frag_shape_bf16(4 * CM, CM, 1),
            _frag_shape_bf16(4 * CM, CIN, 1))
    return all(tuple(f.shape) == w for f, w in zip(frags, want))


def bottleneck_block_bf16(x, frag1, bias1, frag2, bias2, frag3, bias3, out=None):
    """A whole identity-shortcut bottleneck block in one launch (tspn_bottleneck_block_bf16):
    relu(conv1x1(relu(conv3x3(relu(conv1x1(x) + b1)) + b2)) + b3 + x) for x bf16 [NB,H,W,4 CM], CM in (64, 128);
    frag1 / frag2 / frag3 = pack_conv2d_frag_bf16 of the folded conv1 [CM,4CM,1,1], conv2 [CM,CM,3,3], conv3 [4CM,CM,1,1].
    Bit-identical to conv2d_nhwc_bf16 (conv1) + bottleneck_tail_bf16; the 4 CM-channel map is read once."""
    _block_operands(x, (frag1, frag2, frag3), (bias1, bias2, bias3))
    NB, H, W, C4 = x.shape
    CM = C4 // 4
    if CM not in (64, 128) or C4 != 4 * CM:
        raise ValueError(f"bottleneck_block_bf16: needs 4 x 64 or 4 x 128 channels (got {C4})")
    if not _block_frags_match((frag1, frag2, frag3), C4, CM):
        raise ValueError("bottleneck_block_bf16: frag1 / frag2 / frag3 must be pack_conv2d_frag_bf16 of [CM,4CM,1,1] / "
                         "[CM,CM,3,3] / [4CM,CM,1,1]")
    if bias1.shape != (CM,) or bias2.shape != (CM,) or bias3.shape != (C4,):
        raise ValueError("bottleneck_block_bf16: bias shape mismatch")
    out = _out_bf16(out, x.shape, x.device, "bottleneck_block_bf16")
    _abi.check(_abi.lib().tspn_bottleneck_block_bf16(_p(x), NB, H, W, CM, _p(frag1), _p(bias1), _p(frag2), _p(bias2),
                                                     _p(frag3), _p(bias3), _p(out), _stream()))
    return out


def bottleneck_block_proj_bf16(x, stride, frag1, bias1, frag2, bias2, frag3, bias3, frags, biass, out=None):
    """The first block of a stage in one launch (tspn_bottleneck_block_proj_bf16): conv1 and the projection shortcut are
    1x1 convs of stride `stride` on x bf16 [NB,Hin,Win,CIN]; frags / biass = the folded shortcut [4CM,CIN,1,1].  Built for
    (CIN, CM, stride) = (64, 64, 1), detectron2's res2.0.  Bit-identical to conv1 + shortcut + fused tail; the shortcut map
    never goes to memory."""
    _block_operands(x, (frag1, frag2, frag3, frags), (bias1, bias2, bias3, biass))
    NB, Hin, Win, CIN = x.shape
    CM = frag2.shape[0] * 32
    if (CIN, CM, int(stride)) != (64, 64, 1):
        raise ValueError(f"bottleneck_block_proj_bf16: built for (CIN, CM, stride) = (64, 64, 1), got {(CIN, CM, stride)}")
    if not _block_frags_match((frag1, frag2, frag3, frags), CIN, CM):
        raise ValueError("bottleneck_block_proj_bf16: fragment shapes do not match [CM,CIN,1,1] / [CM,CM,3,3] / [4CM,CM,1,1] / [4CM,CIN,1,1]")
    if bias1.shape != (CM,) or bias2.shape != (CM,) or bias3.shape != (4 * CM,) or biass.shape != (4 * CM,):
        raise ValueError("bottleneck_block_proj_bf16: bias shape mismatch")
    H, W = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    out = _out_bf16(out, (NB, H, W, 4 * CM), x.device, "bottleneck_block_proj_bf16")
    _abi.check(_abi.lib().tspn_bottleneck_block_proj_bf16(_p(x), NB, Hin, Win, CIN, int(stride), CM, _p(frag1), _p(bias1),
                                                          _p(frag2), _p(bias2), _p(frag3), _p(bias3), _p(frags), _p(biass),
                                                          _p(out), _stream()))
    return out


def bottleneck_block_res_bf16(x, stride, frag1, bias1, frag2, bias2, frag3, bias3, residual, out=None):
    """conv1 (1x1, stride `stride`) + 3x3 + expand + `residual` + ReLU in one launch (tspn_bottleneck_block_res_bf16): x bf16
    [NB,Hin,Win,CIN], residual bf16 [NB,H,W,4CM] (e.g. the separately launched projection shortcut).  Built for res3.0:
    (CIN, CM, stride) = (256, 128, 2).  Bit-identical to conv1 + bottleneck_tail_bf16."""
    _block_operands(x, (frag1, frag2, frag3), (bias1, bias2, bias3), residual)
    NB, Hin, Win, CIN = x.shape
    CM = frag2.shape[0] * 32
    if (CIN, CM, int(stride)) != (256, 128, 2):
        raise ValueError(f"bottleneck_block_res_bf16: built for (CIN, CM, stride) = (256, 128, 2), got {(CIN, CM, stride)}")
    if not _block_frags_match((frag1, frag2, frag3), CIN, CM):
        raise ValueError("bottleneck_block_res_bf16: fragment shapes do not match [CM,CIN,1,1] / [CM,CM,3,3] / [4CM,CM,1,1]")
    H, W = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
    if bias1.shape != (CM,) or bias2.shape != (CM,) or bias3.shape != (4 * CM,) or tuple(residual.shape) != (NB, H, W, 4 * CM):
        raise ValueError("bottleneck_block_res_bf16: bias / residual shape mismatch")
    out = _out_bf16(out, (NB, H, W, 4 * CM), x.device, "bottleneck_block_res_bf16")
    _abi.check(_abi.lib().tspn_bottleneck_block_res_bf16(_p(x), NB, Hin, Win, CIN, int(stride), CM, _p(frag1), _p(bias1), _p(frag2),
                                                         _p(bias2), _p(frag3), _p(bias3), _p(residual), _p(out), _stream()))
    return out


def bottleneck_tail_bf16(h1, frag2, bias2, frag3, bias3, residual, out=None, next_frag1=None, next_bias1=None,
                         persistent=False, max_workgroups=0, io_waves=False):
    """relu(conv1x1(relu(conv3x3(h1) + b2)) + b3 + residual) in one launch (tspn_bottleneck_tail_bf16): h1 bf16
    [NB,H,W,CM], CM in (64, 128, 256); frag2 / frag3 = pack_conv2d_frag_bf16 of the folded conv2 / conv3 weights;
    residual bf16 [NB,H,W,4 CM] -> bf16 [NB,H,W,4 CM] (written into `out` when given: a contiguous tensor of that
    shape, e.g. a slice of the caller's result along the first dimension).
    `next_frag1`, `next_bias1` (CM = 256): pack_conv2d_frag_bf16 of the FOLLOWING block's conv1 [CM,4 CM,1,1] and its
    bias: the launch also computes that conv1 on its own output (tspn_bottleneck_tail_next_bf16) and the call returns
    (out, h1_next [NB,H,W,CM]) -- both bit-identical to the separate launches.
    `persistent` (CM = 256): the persistent kernel pipelined across tiles (tspn_bottleneck_tail_pipe_bf16: one
    workgroup per CU, the 3x3 phase of tile t beside the expand / store phase of tile t - 1), same results;
    `max_workgroups` > 0 limits its grid (tests).
    `io_waves` (CM = 256): the role-split kernel (tspn_bottleneck_tail_io_bf16, round 5: four MFMA waves + four waves that
    own the h1 DMA, the residual rows and the stores; what the backbone uses for res4), same results."""
    _dev(h1, "h1", torch.bfloat16); _dev(frag2, "frag2", torch.bfloat16); _dev(frag3, "frag3", torch.bfloat16)
    _dev(bias2, "bias2"); _dev(bias3, "bias3"); _dev(residual, "residual", torch.bfloat16)
    NB, H, W, CM = h1.shape
    if CM not in (64, 128, 256):
        raise ValueError(f"bottleneck_tail_bf16: bottleneck channels must be 64, 128 or 256 (got {CM})")
    if tuple(frag2.shape) != _frag_shape_bf16(CM, CM, 9) or tuple(frag3.shape) != _frag_shape_bf16(4 * CM, CM, 1):
        raise ValueError("bottleneck_tail_bf16: frag2 / frag3 must be pack_conv2d_frag_bf16 of [CM,CM,3,3] / [4CM,CM,1,1]")
    if bias2.shape != (CM,) or bias3.shape != (4 * CM,) or tuple(residual.shape) != (NB, H, W, 4 * CM):
        raise ValueError("bottleneck_tail_bf16: bias / residual shape mismatch")
    out = _out_bf16(out, (NB, H, W, 4 * CM), h1.device, "bottleneck_tail_bf16")
    if io_waves:
        # (CM = 256) the role-split kernel: four MFMA waves + four waves that do all HBM traffic (tspn_bottleneck_tail_io_bf16)
        if CM != 256 or next_frag1 is not None or persistent:
            raise ValueError("bottleneck_tail_bf16: io_waves is built for 256 bottleneck channels, without next_frag1 / persistent")
        _abi.check(_abi.lib().tspn_bottleneck_tail_io_bf16(_p(h1), NB, H, W, CM, _p(frag2), _p(bias2), _p(frag3), _p(bias3),
                                                           _p(residual), _p(out), _stream()))
        return out
    if persistent:
        if CM != 256 or next_frag1 is not None:
            raise ValueError("bottleneck_tail_bf16: the persistent form is built for 256 bottleneck channels, without next_frag1")
        _abi.check(_abi.lib().tspn_bottleneck_tail_pipe_bf16(_p(h1), NB, H, W, CM, _p(frag2), _p(bias2), _p(frag3), _p(bias3),
                                                             _p(residual), _p(out), int(max_workgroups), _stream()))
        return out
    if next_frag1 is not None:
        _dev(next_frag1, "next_frag1", torch.bfloat16); _dev(next_bias1, "next_bias1")
        if CM != 256:
            raise ValueError(f"bottleneck_tail_bf16: the fused next conv1 needs 256 bottleneck channels (got {CM})")
        if tuple(next_frag1.shape) != _frag_shape_bf16(CM, 4 * CM, 1) or next_bias1.shape != (CM,):
            raise ValueError("bottleneck_tail_bf16: next_frag1 must be pack_conv2d_frag_bf16 of [CM,4CM,1,1], next_bias1 [CM]")
        h1n = torch.empty((NB, H, W, CM), dtype=torch.bfloat16, device=h1.device)
        _abi.check(_abi.lib().tspn_bottleneck_tail_next_bf16(
            _p(h1), NB, H, W, CM, _p(frag2), _p(bias2), _p(frag3), _p(bias3), _p(residual), _p(out),
            _p(next_frag1), _p(next_bias1), _p(h1n), _stream()))
        return out, h1n
    _abi.check(_abi.lib().tspn_bottleneck_tail_bf16(_p(h1), NB, H, W, CM, _p(frag2), _p(bias2), _p(frag3), _p(bias3),
                                                    _p(residual), _p(out), _stream()))
    return out


def max_pool_nhwc_bf16(x, kernel_size=3, stride=2, padding=1):
    """max_pool2d on a channels-last bf16 map [NB,H,W,C] -> bf16 [NB,OH,OW,C] (tspn_max_pool_nhwc_bf16; C % 8 == 0)."""
    _dev(x, "x", torch.bfloat16)
    NB, H, W, C = x.shape
    OH, OW = _out_hw("max_pool_nhwc_bf16", H, W, kernel_size, kernel_size, stride, padding)
    out = torch.empty((NB, OH, OW, C), dtype=torch.bfloat16, device=x.device)
    _abi.check(_abi.lib().tspn_max_pool_nhwc_bf16(_p(x), NB, H, W, C, kernel_size, stride, padding, _p(out), _stream()))
    return out


def pack_stem_bf16(weight):
    """Stem weight [Cout in (32, 64), 3, 7, 7] fp32 (batch norm folded) -> bf16 fragment-major [Cout/32, 16, 64, 8]
    (tspn_pack_stem_bf16: the 7x7/2 conv as a 4x4/1 conv on the 2x2 space-to-depth image)."""
    _dev(weight, "stem weight")
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (3, 7, 7) or weight.shape[0] not in (32, 64):
        raise ValueError(f"pack_stem_bf16: weight must be [32 | 64, 3, 7, 7], got {tuple(weight.shape)}")
    frag = torch.empty((weight.shape[0] // 32, 16, 64, 8), dtype=torch.bfloat16, device=weight.device)
    _abi.check(_abi.lib().tspn_pack_stem_bf16(_p(weight), weight.shape[0], _p(frag), _stream()))
    return frag


def _stem_bf16(who, pooled, x, frag, bias, workspace):
    """stem_conv_bf16 and, `pooled`, stem_pool_bf16: one body, the entry tspn_<who> and the output's size apart."""
    _dev(x, "x"); _dev(frag, "frag", torch.bfloat16); _dev(bias, "bias")
    if x.dim() != 4 or x.shape[3] != 3 or frag.dim() != 4 or tuple(frag.shape[1:]) != (16, 64, 8):
        raise ValueError(f"{who}: x must be [NB,H,W,3] and frag = pack_stem_bf16(weight)")
    NB, H, W, _ = x.shape
    Cout = frag.shape[0] * 32
    if bias.shape != (Cout,):
        raise ValueError(f"{who}: bias shape mismatch")
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if pooled:
        OH, OW = (OH - 1) // 2 + 1, (OW - 1) // 2 + 1
    l = _abi.lib()
    workspace = _workspace(workspace, l.tspn_stem_bf16_workspace_bytes(NB, H, W), x.device, who)
    out = torch.empty((NB, OH, OW, Cout), dtype=torch.bfloat16, device=x.device)
    _abi.check(getattr(l, "tspn_" + who)(_p(x), NB, H, W, _p(frag), Cout, _p(bias), _p(workspace),
                                         workspace.numel() * workspace.element_size(), _p(out), _stream()))
    return out


def stem_conv_bf16(x, frag, bias, workspace=None):
    """relu(conv7x7/2/pad3(x) + bias) with bf16 operands: x fp32 [NB,H,W,3] -> bf16 [NB,OH,OW,Cout]
    (tspn_stem_conv_bf16; `workspace` >= tspn_stem_bf16_workspace_bytes holds the space-to-depth image)."""
    return _stem_bf16("stem_conv_bf16", False, x, frag, bias, workspace)


def stem_pool_bf16(x, frag, bias, workspace=None):
    """BasicStem.forward on bf16 operands in one conv launch: max_pool2d(relu(conv7x7/2/pad3(x) + bias), 3, 2, 1),
    x fp32 [NB,H,W,3] -> bf16 [NB,PH,PW,Cout] (tspn_stem_pool_bf16); bit-identical to
    max_pool_nhwc_bf16(stem_conv_bf16(x, frag, bias), 3, 2, 1) without writing the conv map."""
    return _stem_bf16("stem_pool_bf16", True, x, frag, bias, workspace)


def pack_conv2d_frag_cin4(weight):
    """Stem weights [Cout, Cin <= 4, KH, KW] -> [Cout/32, ceil(KH*KW/4), 64, 8] (tspn_pack_conv2d_frag_cin4_f32)."""
    _dev(weight, "conv2d weight")
    Cout, Cin, KH, KW = weight.shape
    if Cin > 4 or Cout % 32:
        raise ValueError(f"pack_conv2d_frag_cin4: needs Cin <= 4 and Cout % 32 == 0 (Cin={Cin}, Cout={Cout})")
    frag = torch.empty((Cout // 32, (KH * KW + 3) // 4, 64, 8), dtype=torch.float32, device=weight.device)
    _abi.check(_abi.lib().tspn_pack_conv2d_frag_cin4_f32(_p(weight), Cout, Cin, KH, KW, _p(frag), _stream()))
    return frag


def conv2d_nhwc_cin4(x, frag, kernel_size, stride=1, padding=0, bias=None, relu=False):
    """Stem conv on a 4-channel channels-last image x [NB,H,W,4] (RGB + one zero channel) -> [NB,OH,OW,Cout]."""
    _dev(x, "x"); _dev(frag, "frag")
    NB, H, W, C4 = x.shape
    KH, KW = kernel_size
    if C4 != 4 or frag.dim() != 4 or tuple(frag.shape[1:]) != ((KH * KW + 3) // 4, 64, 8):
        raise ValueError("conv2d_nhwc_cin4: x must be [NB,H,W,4] and frag = pack_conv2d_frag_cin4(weight)")
    Cout = frag.shape[0] * 32
    OH, OW = _out_hw("conv2d_nhwc_cin4", H, W, KH, KW, stride, padding)
    if bias is not None:
        _dev(bias, "bias")
    out = torch.empty((NB, OH, OW, Cout), dtype=torch.float32, device=x.device)
    _abi.check(_abi.lib().tspn_conv2d_nhwc_cin4_f32(_p(x), NB, H, W, _p(frag), Cout, KH, KW, stride, padding,
                                                    _p(bias), 1 if relu else 0, _p(out), _stream()))
    return out



# ---- video relation detection evaluation (csrc/eval/tspn_eval.hip; packed by evaluation.py)
def _eval_traj(boxes, traj):
    _dev(boxes, "boxes", torch.float64), _dev(traj, "traj", torch.int64)
    if boxes.dim() != 2 or boxes.shape[1] != 4 or traj.dim() != 2 or traj.shape[1] != 3:
        raise ValueError(f"eval: boxes [F,4] and traj [T,3] expected, got {tuple(boxes.shape)} and {tuple(traj.shape)}")
    if boxes.data_ptr() % 32:
        raise ValueError("eval: boxes must be 32-byte aligned")
    return traj.shape[0]


def eval_traj_volume(boxes, traj, out=None):
    """Volume of every packed trajectory: boxes [F,4] float64, traj [T,3] int64 (row offset, begin, end) -> [T]
    float64, summed in frame order like the reference's viou (lib/evaluation/common.py:100-105)."""
    T = _eval_traj(boxes, traj)
    if out is None:
        out = torch.empty(T, dtype=torch.float64, device=boxes.device)
    elif _dev(out, "out", torch.float64).shape != (T,):
        raise ValueError(f"eval_traj_volume: out must be [{T}]")
    _abi.check(_abi.lib().tspn_eval_traj_volume_f64(_p(boxes), _p(traj), T, _p(out), _stream()))
    return out


def eval_viou(boxes, traj, vol, groups, pred_group, n_cand, ov=None, zden=None):
    """ov [n_cand] float64 = min(subject vIoU, object vIoU) of every (prediction, same-triplet ground truth) pair,
    group blocks row-major (include/tspn_mi355x.h); zden [P] int32 = 1 where a pair had a zero vIoU denominator.
    groups [G,5] int64, pred_group [P] int32.  Returns (ov, zden)."""
    T = _eval_traj(boxes, traj)
    _dev(vol, "vol", torch.float64), _dev(groups, "groups", torch.int64), _dev(pred_group, "pred_group", torch.int32)
    if vol.shape != (T,) or groups.dim() != 2 or groups.shape[1] != 5 or pred_group.dim() != 1:
        raise ValueError("eval_viou: vol [T], groups [G,5] and pred_group [P] expected")
    P = pred_group.shape[0]
    if 2 * P > T:
        raise ValueError(f"eval_viou: {P} predictions need {2 * P} trajectories, traj has {T}")
    dev = boxes.device
    ov = torch.empty(int(n_cand), dtype=torch.float64, device=dev) if ov is None else _dev(ov, "ov", torch.float64)
    zden = torch.empty(P, dtype=torch.int32, device=dev) if zden is None else _dev(zden, "zden", torch.int32)
    if ov.shape != (int(n_cand),) or zden.shape != (P,):
        raise ValueError(f"eval_viou: ov must be [{n_cand}] and zden [{P}]")
    _abi.check(_abi.lib().tspn_eval_viou_f64(_p(boxes), _p(traj), _p(vol), _p(groups), _p(pred_group), P, _p(ov),
                                             _p(zden), _stream()))
    return ov, zden


def eval_greedy_match(ov, groups, n_pred, viou_threshold, max_group_gt, det_ws=None, hit=None, match=None):
    """The reference's greedy match per (video, triplet) group: hit [n_pred] int8 (0/1) and match [n_pred] int32
    (ground-truth index inside the group, -1 for none).  max_group_gt: the largest group's ground-truth count; above
    4096 `det_ws` (uint8, one zeroed byte per packed relation) is required.  Returns (hit, match)."""
    _dev(ov, "ov", torch.float64), _dev(groups, "groups", torch.int64)
    if groups.dim() != 2 or groups.shape[1] != 5 or ov.dim() != 1:
        raise ValueError("eval_greedy_match: ov [C] and groups [G,5] expected")
    if det_ws is not None:
        _dev(det_ws, "det_ws", torch.uint8)
    elif max_group_gt > 4096:
        raise ValueError("eval_greedy_match: groups of more than 4096 ground truths need det_ws")
    dev = ov.device
    hit = torch.empty(int(n_pred), dtype=torch.int8, device=dev) if hit is None else _dev(hit, "hit", torch.int8)
    match = torch.empty(int(n_pred), dtype=torch.int32, device=dev) if match is None else _dev(match, "match", torch.int32)
    if hit.shape != (int(n_pred),) or match.shape != (int(n_pred),):
        raise ValueError(f"eval_greedy_match: hit and match must be [{n_pred}]")
    _abi.check(_abi.lib().tspn_eval_greedy_match_f64(_p(ov), _p(groups), groups.shape[0], int(max_group_gt),
                                                     float(viou_threshold), _p(det_ws), _p(hit), _p(match), _stream()))
    return hit, match


# ---- video object detection evaluation (csrc/evalobj/tspn_eval_objects.hip; packed by evaluation_detection.py)
def _evalobj_groups(who, groups, pred_group):
    _dev(groups, "groups", torch.int64), _dev(pred_group, "pred_group", torch.int32)
    if groups.dim() != 2 or groups.shape[1] != 5 or pred_group.dim() != 1:
        raise ValueError(f"{who}: groups [G,5] and pred_group [P] expected, got {tuple(groups.shape)} and "
                         f"{tuple(pred_group.shape)}")
    if pred_group.shape[0] and not groups.shape[0]:
        raise ValueError(f"{who}: {pred_group.shape[0]} predictions and no group")
    return pred_group.shape[0]


def _evalobj_out(who, t, name, n, dtype, dev):
    if t is None:
        return torch.empty(int(n), dtype=dtype, device=dev)
    if _dev(t, name, dtype).shape != (int(n),):
        raise ValueError(f"{who}: {name} must be [{int(n)}]")
    return t


def evalobj_tiou(boxes, frames, traj, groups, pred_group, n_cand=None, tiou=None, best=None, best_index=None, flags=None):
    """The reference's trajectory overlap (video_object_detection.py:12-43) of every prediction of a packed chunk against
    the ground truths of its (video, class) group: boxes [F,4] float64, frames [F] int32 (ascending inside a trajectory),
    traj [T,2] int64 (first row, rows), groups [G,5] int64, pred_group [P] int32 (include/tspn_mi355x.h).  Returns
    (tiou, best, best_index, flags): tiou [n_cand] float64, every pair's tIoU in row-major group blocks (None unless
    `n_cand` or `tiou` is given), best [P] float64 and best_index [P] int32 (max_overlap, max_index), flags [P] int32
    (bit 0: a zero sIoU denominator, bit 1: a pair of two empty trajectories)."""
    who = "evalobj_tiou"
    _dev(boxes, "boxes", torch.float64), _dev(frames, "frames", torch.int32), _dev(traj, "traj", torch.int64)
    if boxes.dim() != 2 or boxes.shape[1] != 4 or frames.shape != (boxes.shape[0],) or traj.dim() != 2 or traj.shape[1] != 2:
        raise ValueError(f"{who}: boxes [F,4], frames [F] and traj [T,2] expected, got {tuple(boxes.shape)}, "
                         f"{tuple(frames.shape)} and {tuple(traj.shape)}")
    if boxes.data_ptr() % 32:
        raise ValueError(f"{who}: boxes must be 32-byte aligned")
    P = _evalobj_groups(who, groups, pred_group)
    if P > traj.shape[0]:
        raise ValueError(f"{who}: {P} predictions need {P} trajectories, traj has {traj.shape[0]}")
    dev = boxes.device
    if tiou is not None or n_cand is not None:
        tiou = _evalobj_out(who, tiou, "tiou", tiou.shape[0] if n_cand is None else n_cand, torch.float64, dev)
    best = _evalobj_out(who, best, "best", P, torch.float64, dev)
    best_index = _evalobj_out(who, best_index, "best_index", P, torch.int32, dev)
    flags = _evalobj_out(who, flags, "flags", P, torch.int32, dev)
    _abi.check(_abi.lib().tspn_evalobj_tiou_f64(_p(boxes), _p(frames), _p(traj), _p(groups), _p(pred_group), P, _p(tiou),
                                                _p(best), _p(best_index), _p(flags), _stream()))
    return tiou, best, best_index, flags


def evalobj_claim(best, best_index, groups, pred_group, n_gt, thresh_t, claim=None, hit=None):
    """The reference's true-positive rule (video_object_detection.py:93-106) from `evalobj_tiou`'s best / best_index: a
    prediction with best >= thresh_t claims its ground truth with its position inside its group, the smallest position
    wins.  Returns (claim, hit): claim [n_gt] int32 (INT32_MAX: unclaimed; written in full by the call), hit [P] int8."""
    who = "evalobj_claim"
    _dev(best, "best", torch.float64), _dev(best_index, "best_index", torch.int32)
    P = _evalobj_groups(who, groups, pred_group)
    if best.shape != (P,) or best_index.shape != (P,):
        raise ValueError(f"{who}: best and best_index must be [{P}]")
    if int(n_gt) < 0 or not float(thresh_t) == float(thresh_t):
        raise ValueError(f"{who}: n_gt must be >= 0 and thresh_t a number")
    claim = _evalobj_out(who, claim, "claim", n_gt, torch.int32, best.device)
    hit = _evalobj_out(who, hit, "hit", P, torch.int8, best.device)
    _abi.check(_abi.lib().tspn_evalobj_claim(_p(best), _p(best_index), _p(groups), _p(pred_group), P, int(n_gt),
                                             float(thresh_t), _p(claim), _p(hit), _stream()))
    return claim, hit


# ---- per-frame object detection: RPN proposals, box head, box NMS (csrc/detect/tspn_detect.hip)
def _image_sizes(who, image_sizes, B):
    if _dev(image_sizes, "image_sizes").shape != (B, 2):
        raise ValueError(f"{who}: image_sizes must be fp32 [{B}, 2] = (height, width), got {tuple(image_sizes.shape)}")


def _group_off(who, group_off):
    """Host group offsets (a sequence or a CPU tensor of G + 1 ascending integers) as the int64 array the C entry reads."""
    if isinstance(group_off, torch.Tensor):
        if group_off.is_cuda:
            raise ValueError(f"{who}: group_off lives in host memory (the entry checks it before it launches)")
        group_off = group_off.tolist()
    vals = [int(v) for v in group_off]
    if not vals:
        raise ValueError(f"{who}: group_off needs G + 1 entries")
    return (ctypes.c_int64 * len(vals))(*vals), len(vals) - 1


def box_nms_workspace_bytes(group_off, pre_topk, select_only=False):
    """Bytes of scratch tspn_box_nms_f32 needs for these groups (0: a shape it refuses, or no group)."""
    arr, G = _group_off("box_nms_workspace_bytes", group_off)
    return int(_abi.lib().tspn_box_nms_scratch_bytes(arr, G, int(pre_topk), 1 if select_only else 0))


def box_nms(boxes, scores, group_off, pre_topk, iou_threshold, post_topk, min_size=-1.0, valid=None, want_keep=False,
            workspace=None):
    """Greedy 2-D box NMS per contiguous group (tspn_box_nms_f32): boxes fp32 [n,4] (None: the selection alone), scores fp32
    [n], valid uint8 [n] or None, group_off G + 1 host offsets ascending from 0 to n.  Per group: the pre_topk best scores
    in selection order, invalid rows and (min_size >= 0) boxes not larger than min_size dropped, torchvision's NMS at
    iou_threshold, the first post_topk survivors.  Returns (index int64 [G, post_topk] of flat candidate indices, -1 past
    the count; count int64 [G]; keep uint8 [n] or None).  No host synchronisation."""
    who = "box_nms"
    _dev(scores, "scores")
    n = scores.shape[0]
    if scores.dim() != 1:
        raise ValueError(f"{who}: scores must be [n]")
    if boxes is not None and tuple(_dev(boxes, "boxes").shape) != (n, 4):
        raise ValueError(f"{who}: boxes must be [{n}, 4], got {tuple(boxes.shape)}")
    if valid is not None and tuple(_dev(valid, "valid", torch.uint8).shape) != (n,):
        raise ValueError(f"{who}: valid must be uint8 [{n}]")
    arr, G = _group_off(who, group_off)
    pre_topk, post_topk = int(pre_topk), int(post_topk)
    l = _abi.lib()
    dev = scores.device
    index = torch.empty((G, max(post_topk, 0)), dtype=torch.int64, device=dev)
    count = torch.empty((G,), dtype=torch.int64, device=dev)
    keep = torch.empty((n,), dtype=torch.uint8, device=dev) if (want_keep and boxes is not None) else None
    need = l.tspn_box_nms_scratch_bytes(arr, G, pre_topk, 1 if boxes is None else 0)
    ws = _workspace(workspace, need, dev, who, sizes=True)
    _abi.check(l.tspn_box_nms_f32(_p(boxes), _p(scores), _p(valid), n, arr, G, pre_topk, float(iou_threshold), post_topk,
                                  float(min_size), _p(index), _p(count), _p(keep), _p(ws),
                                  ws.numel() * ws.element_size(), _stream()))
    return index, count, keep


def rpn_decode(cand, logits, deltas, cell_anchors, stride, image_sizes):
    """Anchors + RPN deltas -> clipped boxes (tspn_rpn_decode_f32): logits fp32 [B,H,W,A], deltas fp32 [B,H,W,4A] (channel
    4a + k), cell_anchors fp32 [A,4], image_sizes fp32 [B,2] = (height, width); cand int64 [B,M] of flat indices
    b HWA + (h W + w) A + a (None: every anchor).  Returns (boxes [B,M,4], logits [B,M], valid uint8 [B,M])."""
    who = "rpn_decode"
    _dev(logits, "logits"), _dev(deltas, "deltas"), _dev(cell_anchors, "cell_anchors")
    if logits.dim() != 4 or cell_anchors.shape != (logits.shape[3], 4) or \
            tuple(deltas.shape) != tuple(logits.shape[:3]) + (4 * logits.shape[3],):
        raise ValueError(f"{who}: logits [B,H,W,A], deltas [B,H,W,4A] and cell_anchors [A,4] expected, got "
                         f"{tuple(logits.shape)}, {tuple(deltas.shape)} and {tuple(cell_anchors.shape)}")
    B, H, W, A = logits.shape
    _image_sizes(who, image_sizes, B)
    if cand is not None and (_dev(cand, "cand", torch.int64).dim() != 2 or cand.shape[0] != B):
        raise ValueError(f"{who}: cand must be int64 [{B}, M]")
    M = H * W * A if cand is None else cand.shape[1]
    dev = logits.device
    boxes = torch.empty((B, M, 4), dtype=torch.float32, device=dev)
    out_logits = torch.empty((B, M), dtype=torch.float32, device=dev)
    valid = torch.empty((B, M), dtype=torch.uint8, device=dev)
    _abi.check(_abi.lib().tspn_rpn_decode_f32(_p(cand), _p(logits), _p(deltas), _p(cell_anchors), _p(image_sizes), B, H, W, A,
                                              M, float(stride), _p(boxes), _p(out_logits), _p(valid), _stream()))
    return boxes, out_logits, valid


def box_head_decode(cls_logits, deltas, proposals, proposal_count, image_sizes, score_thresh=0.05,
                    weights=(10.0, 10.0, 5.0, 5.0)):
    """Softmax scores and class-specific boxes of the box head (tspn_box_head_decode_f32): cls_logits fp32 [B R, K+1]
    (background last), deltas fp32 [B R, 4K], proposals fp32 [B,R,4], proposal_count int64 [B].  Returns class-major
    (scores [B,K,R], boxes [B,K,R,4], valid uint8 [B,K,R]); where valid is 0 the score is 0."""
    who = "box_head_decode"
    _dev(cls_logits, "cls_logits"), _dev(deltas, "deltas"), _dev(proposals, "proposals")
    if proposals.dim() != 3 or proposals.shape[2] != 4:
        raise ValueError(f"{who}: proposals must be [B,R,4], got {tuple(proposals.shape)}")
    B, R, _ = proposals.shape
    if cls_logits.dim() != 2 or cls_logits.shape[0] != B * R or cls_logits.shape[1] < 2 or \
            tuple(deltas.shape) != (B * R, 4 * (cls_logits.shape[1] - 1)):
        raise ValueError(f"{who}: cls_logits [{B * R}, K+1] and deltas [{B * R}, 4K] expected, got "
                         f"{tuple(cls_logits.shape)} and {tuple(deltas.shape)}")
    K = cls_logits.shape[1] - 1
    if _dev(proposal_count, "proposal_count", torch.int64).shape != (B,):
        raise ValueError(f"{who}: proposal_count must be int64 [{B}]")
    _image_sizes(who, image_sizes, B)
    dev = proposals.device
    scores = torch.empty((B, K, R), dtype=torch.float32, device=dev)
    boxes = torch.empty((B, K, R, 4), dtype=torch.float32, device=dev)
    valid = torch.empty((B, K, R), dtype=torch.uint8, device=dev)
    wx, wy, ww, wh = (float(v) for v in weights)
    _abi.check(_abi.lib().tspn_box_head_decode_f32(_p(cls_logits), _p(deltas), _p(proposals), _p(proposal_count),
                                                   _p(image_sizes), B, R, K, wx, wy, ww, wh, float(score_thresh),
                                                   _p(scores), _p(boxes), _p(valid), _stream()))
    return scores, boxes, valid


def detections_topk(scores, boxes, keep, detections_per_image=100):
    """Per image the best NMS survivors over all classes (tspn_detections_topk_f32): scores [B,K,R], boxes [B,K,R,4], keep
    uint8 [B,K,R] -> (boxes [B,D,4], scores [B,D], classes int64 [B,D], count int64 [B]); ties to the lower r K + c."""
    who = "detections_topk"
    _dev(scores, "scores"), _dev(boxes, "boxes"), _dev(keep, "keep", torch.uint8)
    if scores.dim() != 3 or tuple(boxes.shape) != tuple(scores.shape) + (4,) or keep.shape != scores.shape:
        raise ValueError(f"{who}: scores [B,K,R], boxes [B,K,R,4] and keep [B,K,R] expected")
    B, K, R = scores.shape
    D = int(detections_per_image)
    dev = scores.device
    ob = torch.empty((B, D, 4), dtype=torch.float32, device=dev)
    osc = torch.empty((B, D), dtype=torch.float32, device=dev)
    oc = torch.empty((B, D), dtype=torch.int64, device=dev)
    cnt = torch.empty((B,), dtype=torch.int64, device=dev)
    _abi.check(_abi.lib().tspn_detections_topk_f32(_p(scores), _p(boxes), _p(keep), B, K, R, D, _p(ob), _p(osc), _p(oc),
                                                   _p(cnt), _stream()))
    return ob, osc, oc, cnt


def rpn_proposals(logits, deltas, cell_anchors, stride, image_sizes, pre_nms_topk=6000, post_nms_topk=1000, nms_thresh=0.7,
                  min_size=0.0, workspace=None):
    """detectron2's find_top_rpn_proposals (eval) on one feature level: per image the pre_nms_topk best logits, decoded,
    non-finite rows dropped, clipped, boxes not larger than min_size dropped, NMS at nms_thresh, the first post_nms_topk.
    Returns (boxes [B,post,4], logits [B,post], count int64 [B]); rows past the count are zero.  No host synchronisation."""
    who = "rpn_proposals"
    _dev(logits, "logits")
    if logits.dim() != 4:
        raise ValueError(f"{who}: logits must be [B,H,W,A]")
    B = logits.shape[0]
    HWA = logits.shape[1] * logits.shape[2] * logits.shape[3]
    M = min(int(pre_nms_topk), HWA)
    post = min(int(post_nms_topk), M)
    sel_off, nms_off = range(0, (B + 1) * HWA, HWA), range(0, (B + 1) * M, M)
    need = max(box_nms_workspace_bytes(sel_off, M, True), box_nms_workspace_bytes(nms_off, M))
    ws = _workspace(workspace, need, logits.device, who, sizes=True)
    cand, _, _ = box_nms(None, logits.reshape(-1), sel_off, M, 0.0, M, workspace=ws)
    boxes, lg, valid = rpn_decode(cand, logits, deltas, cell_anchors, stride, image_sizes)
    index, count, _ = box_nms(boxes.view(-1, 4), lg.view(-1), nms_off, M, nms_thresh, post, min_size=min_size,
                              valid=valid.view(-1), workspace=ws)
    live = index >= 0
    at = index.clamp(min=0)
    out_boxes = torch.zeros((B, int(post_nms_topk), 4), dtype=torch.float32, device=logits.device)
    out_logits = torch.zeros((B, int(post_nms_topk)), dtype=torch.float32, device=logits.device)
    out_boxes[:, :post] = torch.where(live[..., None], boxes.view(-1, 4)[at], out_boxes[:, :post])
    out_logits[:, :post] = torch.where(live, lg.view(-1)[at], out_logits[:, :post])
    return out_boxes, out_logits, count


def box_detections(cls_logits, deltas, proposals, proposal_count, image_sizes, score_thresh=0.05, nms_thresh=0.5,
                   detections_per_image=100, weights=(10.0, 10.0, 5.0, 5.0), workspace=None):
    """detectron2's fast_rcnn_inference per image: softmax, class-specific boxes, clip, score > score_thresh, NMS per class
    at nms_thresh, the detections_per_image best over all classes.  Returns (boxes [B,D,4], scores [B,D], classes int64
    [B,D], count int64 [B]).  No host synchronisation."""
    scores, boxes, valid = box_head_decode(cls_logits, deltas, proposals, proposal_count, image_sizes, score_thresh, weights)
    B, K, R = scores.shape
    if R == 0:
        raise ValueError("box_detections: no proposal rows (R = 0)")
    _, _, keep = box_nms(boxes.view(-1, 4), scores.view(-1), range(0, (B * K + 1) * R, R), R, nms_thresh, R, min_size=-1.0,
                         valid=valid.view(-1), want_keep=True, workspace=workspace)
    return detections_topk(scores, boxes, keep.view(B, K, R), detections_per_image)


# ---- tracklet linking: detections -> tracks -> dense tracklet boxes (csrc/link/tspn_link.hip)
def _link_operands(who, boxes, video_off):
    if _dev(boxes, "boxes").dim() != 3 or boxes.shape[2] != 4:
        raise ValueError(f"{who}: boxes must be fp32 [F, D, 4], got {tuple(boxes.shape)}")
    F, D = boxes.shape[:2]
    arr, V = _group_off(who, [0, F] if video_off is None else video_off)
    return F, D, arr, V


def link_detections(boxes, scores, classes, count, video_off=None, iou_thresh=0.3, max_age=30, min_hits=3, min_score=0.0,
                    class_aware=True, max_live=1024, max_tracks=16384, workspace=None):
    """The link pass (tspn_link_detections_f32) over the outputs of FasterRCNNC4.forward: boxes fp32 [F,D,4], scores fp32
    [F,D], classes int64 [F,D], count int64 [F]; video_off V + 1 host frame offsets ascending from 0 to F (None: one
    video).  A deterministic IoU tracker with constant-velocity prediction ("tracklet linking").  Returns
    (track_of_det int32 [F,D], n_tracks int64 [V], dropped int64 [V], first, last, hits int32 [V,max_tracks], cls int64
    [V,max_tracks], score fp32 [V,max_tracks]); frames count from the video's first.  No host synchronisation."""
    who = "link_detections"
    F, D, arr, V = _link_operands(who, boxes, video_off)
    if tuple(_dev(scores, "scores").shape) != (F, D) or tuple(_dev(classes, "classes", torch.int64).shape) != (F, D) or \
            tuple(_dev(count, "count", torch.int64).shape) != (F,):
        raise ValueError(f"{who}: scores [{F}, {D}], classes int64 [{F}, {D}] and count int64 [{F}] expected, got "
                         f"{tuple(scores.shape)}, {tuple(classes.shape)} and {tuple(count.shape)}")
    max_live, max_tracks = int(max_live), int(max_tracks)
    dev = boxes.device
    l = _abi.lib()
    tod = torch.empty((F, D), dtype=torch.int32, device=dev)
    n_tracks = torch.empty((V,), dtype=torch.int64, device=dev)
    dropped = torch.empty((V,), dtype=torch.int64, device=dev)
    shape = (V, max(max_tracks, 0))
    first, last, hits = (torch.empty(shape, dtype=torch.int32, device=dev) for _ in range(3))
    cls = torch.empty(shape, dtype=torch.int64, device=dev)
    score = torch.empty(shape, dtype=torch.float32, device=dev)
    need = l.tspn_link_scratch_bytes(V, max_live, max_tracks, 0, 0, 0)
    ws = _workspace(workspace, need, dev, who, sizes=True)
    _abi.check(l.tspn_link_detections_f32(_p(boxes), _p(scores), _p(classes), _p(count), arr, V, F, D, float(iou_thresh),
                                          int(max_age), int(min_hits), float(min_score), 1 if class_aware else 0, max_live,
                                          max_tracks, _p(tod), _p(n_tracks), _p(dropped), _p(first), _p(last), _p(hits),
                                          _p(cls), _p(score), _p(ws), ws.numel() * ws.element_size(), _stream()))
    return tod, n_tracks, dropped, first, last, hits, cls, score


def link_fill(boxes, track_of_det, first, last, sel_video, sel_track, video_off=None, workspace=None):
    """The fill pass (tspn_link_fill_f32): dense boxes of the selected tracks (sel_video, sel_track int64 [R] on the
    device) from the detections and the link pass's track_of_det and first / last tables.  Returns (track_boxes fp32
    [R,Fmax,4], state uint8 [R,Fmax]: 0 absent, 1 detected, 2 interpolated), Fmax the longest video."""
    who = "link_fill"
    F, D, arr, V = _link_operands(who, boxes, video_off)
    if tuple(_dev(track_of_det, "track_of_det", torch.int32).shape) != (F, D):
        raise ValueError(f"{who}: track_of_det must be int32 [{F}, {D}]")
    _dev(first, "first", torch.int32), _dev(last, "last", torch.int32)
    if first.dim() != 2 or first.shape[0] != V or last.shape != first.shape:
        raise ValueError(f"{who}: first and last must be int32 [{V}, max_tracks]")
    _dev(sel_video, "sel_video", torch.int64), _dev(sel_track, "sel_track", torch.int64)
    if sel_video.dim() != 1 or sel_track.shape != sel_video.shape:
        raise ValueError(f"{who}: sel_video and sel_track must be int64 [R]")
    R, max_tracks = sel_video.shape[0], first.shape[1]
    Fmax = max([arr[v + 1] - arr[v] for v in range(V)] + [0])
    dev = boxes.device
    l = _abi.lib()
    out = torch.empty((R, Fmax, 4), dtype=torch.float32, device=dev)
    state = torch.empty((R, Fmax), dtype=torch.uint8, device=dev)
    need = l.tspn_link_scratch_bytes(V, 1, max_tracks, R, Fmax, 1)
    ws = _workspace(workspace, need, dev, who, sizes=True)
    _abi.check(l.tspn_link_fill_f32(_p(boxes), _p(track_of_det), arr, V, F, D, _p(first), _p(last), max_tracks, _p(sel_video),
                                    _p(sel_track), R, _p(out), _p(state), _p(ws), ws.numel() * ws.element_size(), _stream()))
    return out, state


# every public operator runs with the device of its operands made current (see _on_tensor_device)
for _name in __all__:
    if _name not in ("pair_index", "fused_workspace_bytes") and not _name.startswith("status_"):
        globals()[_name] = _on_tensor_device(globals()[_name])
del _name
