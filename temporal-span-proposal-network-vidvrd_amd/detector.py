"""Per-frame object detection on the GPU: the rest of detectron2 v0.6's `faster_rcnn_R_101_C4` around the two modules
of roi_head.py -- the model the reference configures in lib/detectron/trainer.py:23-33 (35 classes) and owns no code for.

    frames -> ResNetC4 -> res4 maps -> RPNHead -> ops.rpn_proposals -> Res5RoIHead -> BoxPredictor -> ops.box_detections

`FasterRCNNC4` keeps detectron2's module tree and parameter names (`backbone.*`, `proposal_generator.rpn_head.*`,
`roi_heads.res5.*`, `roi_heads.box_predictor.*`), so the state dict of a detectron2 C4 checkpoint loads with
`strict=True`.  Inference only, no resizing: image coordinates are input coordinates.  Semantics: DESIGN.md 2 "box
decode", "box NMS", "proposals", "detections"; every tensor operation of the path runs in the HIP library."""
import torch
import torch.nn as nn

from . import ops
from .anchor_generator import generate_cell_anchors_2d
from .model import _CachedWeightsMixin, _DeviceCache, _compute_device, _f32
from .roi_head import Res5RoIHead, ResNetC4

__all__ = ["RPNHead", "BoxPredictor", "FasterRCNNC4"]


def _pad_rows(w, b, multiple):
    """Zero rows up to the next multiple: the conv kernels take output channels in 32s."""
    pad = (-w.shape[0]) % multiple
    if pad:
        w = torch.cat([w, w.new_zeros((pad,) + tuple(w.shape[1:]))])
        b = torch.cat([b, b.new_zeros(pad)])
    return w.contiguous(), b.contiguous()


class RPNHead(nn.Module):
    """detectron2 StandardRPNHead: `conv` 3x3 + ReLU, then the 1x1 heads `objectness_logits` (A channels) and
    `anchor_deltas` (4A channels, channel 4a + k).  The two heads run as ONE 1x1 conv of A + 4A output channels, zero-padded
    to the kernels' granularity and packed once per parameter version."""

    def __init__(self, in_channels=1024, num_anchors=15):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, in_channels, 3, 1, 1)
        self.objectness_logits = nn.Conv2d(in_channels, num_anchors, 1)
        self.anchor_deltas = nn.Conv2d(in_channels, 4 * num_anchors, 1)
        for m in (self.conv, self.objectness_logits, self.anchor_deltas):
            nn.init.normal_(m.weight, std=0.01)
            nn.init.constant_(m.bias, 0)
        self.num_anchors = num_anchors
        self._cache = _DeviceCache()

    def _packed(self, dev, bf16):
        pack = ops.pack_conv2d_frag_bf16 if bf16 else ops.pack_conv2d_frag

        def build(ts):
            cw, cb, ow, ob, dw, db = ts
            hw, hb = _pad_rows(torch.cat([ow, dw]), torch.cat([ob, db]), 32)
            return pack(cw.contiguous()), cb.contiguous(), pack(hw), hb
        c, o, d = self.conv, self.objectness_logits, self.anchor_deltas
        return self._cache.get("packed_bf16" if bf16 else "packed", (c.weight, c.bias, o.weight, o.bias, d.weight, d.bias),
                               dev, build)

    def forward(self, x):
        """x channels-last [T,H,W,C], fp32 or bf16 -> (logits fp32 [T,H,W,A], deltas fp32 [T,H,W,4A])."""
        bf16 = x.dtype == torch.bfloat16
        cin = self.conv.weight.shape[1]
        if x.dim() != 4 or x.shape[3] != cin or cin % (64 if bf16 else 32):
            raise ValueError(f"RPNHead: needs a channels-last map of {cin} channels (a multiple of {64 if bf16 else 32}), got "
                             f"{tuple(x.shape)}")
        conv_w, conv_b, head_w, head_b = self._packed(x.device, bf16)
        conv = ops.conv2d_nhwc_bf16 if bf16 else ops.conv2d_nhwc
        h = conv(x.contiguous(), conv_w, (3, 3), 1, 1, bias=conv_b, relu=True)
        y = conv(h, head_w, (1, 1), 1, 0, bias=head_b).float()
        a = self.num_anchors
        return y[..., :a].contiguous(), y[..., a:5 * a].contiguous()


class BoxPredictor(nn.Module):
    """detectron2 FastRCNNOutputLayers' two linear layers, `cls_score` [K+1, C] (background last) and `bbox_pred` [4K, C],
    as one GEMM of 5K + 1 output columns."""

    def __init__(self, input_size=2048, num_classes=35):
        super().__init__()
        self.cls_score = nn.Linear(input_size, num_classes + 1)
        self.bbox_pred = nn.Linear(input_size, 4 * num_classes)
        nn.init.normal_(self.cls_score.weight, std=0.01)
        nn.init.normal_(self.bbox_pred.weight, std=0.001)
        for l in (self.cls_score, self.bbox_pred):
            nn.init.constant_(l.bias, 0)
        self.num_classes = num_classes
        self._cache = _DeviceCache()

    def forward(self, x):
        """x fp32 [R, C] on the HIP device -> (cls_logits [R, K+1], deltas [R, 4K])."""
        c, b = self.cls_score, self.bbox_pred
        w, bias = self._cache.get("fused", (c.weight, c.bias, b.weight, b.bias), x.device,
                                  lambda ts: (torch.cat([ts[0], ts[2]]).contiguous(), torch.cat([ts[1], ts[3]]).contiguous()))
        y = ops.predicate_head(x.contiguous(), w, bias, apply_sigmoid=False)
        k1 = self.num_classes + 1
        return y[:, :k1].contiguous(), y[:, k1:].contiguous()


class _ProposalGenerator(nn.Module):
    """detectron2's RPN as a parameter holder: `rpn_head` (its anchor generator's buffers are not persistent)."""

    def __init__(self, in_channels, num_anchors):
        super().__init__()
        self.rpn_head = RPNHead(in_channels, num_anchors)


class _Res5ROIHeads(Res5RoIHead):
    """detectron2's Res5ROIHeads: `res5` (the blocks of Res5RoIHead) and `box_predictor`."""

    def __init__(self, in_channels, bottleneck_channels, out_channels, num_blocks, num_classes):
        super().__init__(in_channels, bottleneck_channels, out_channels, num_blocks)
        self.box_predictor = BoxPredictor(out_channels, num_classes)


class FasterRCNNC4(_CachedWeightsMixin, nn.Module):
    """detectron2 GeneralizedRCNN with the R-C4 parts, at inference.

    forward(images [T,H,W,3] channels-last, the checkpoint's channel order and value range (BGR 0..255 for the MSRA
    weights), bf16=False) -> (boxes [T,D,4], scores [T,D], classes int64 [T,D], count int64 [T]) on the HIP device, in
    input pixel coordinates, best first; rows past `count` are zero.  `detect_from_maps(feature_maps, image_sizes)` is the
    same from res4 maps [T,Hf,Wf,C] and image sizes fp32 [T,2] = (height, width)."""

    def __init__(self, num_classes=35, depth=101, blocks=None, stem_out=64, res2_out=256, res5_bottleneck=512,
                 res5_out=2048, res5_blocks=3, anchor_sizes=(32, 64, 128, 256, 512), aspect_ratios=(0.5, 1.0, 2.0),
                 pre_nms_topk=6000, post_nms_topk=1000, rpn_nms_thresh=0.7, min_box_size=0.0, score_thresh=0.05,
                 nms_thresh=0.5, detections_per_image=100, bbox_reg_weights=(10.0, 10.0, 5.0, 5.0),
                 pixel_mean=(103.530, 116.280, 123.675), pixel_std=(1.0, 1.0, 1.0), frame_chunk=8):
        super().__init__()
        self.backbone = ResNetC4(depth, stem_out, res2_out, blocks)
        c4 = self.backbone.out_channels
        cell = generate_cell_anchors_2d(anchor_sizes, aspect_ratios)
        self.proposal_generator = _ProposalGenerator(c4, cell.shape[0])
        self.roi_heads = _Res5ROIHeads(c4, res5_bottleneck, res5_out, res5_blocks, num_classes)
        # detectron2 registers these three as non-persistent buffers: they are not part of a checkpoint
        self.register_buffer("pixel_mean", torch.tensor(pixel_mean, dtype=torch.float32).view(-1, 1, 1), persistent=False)
        self.register_buffer("pixel_std", torch.tensor(pixel_std, dtype=torch.float32).view(-1, 1, 1), persistent=False)
        self.register_buffer("cell_anchors", cell, persistent=False)
        self.stride = 16
        self.pre_nms_topk, self.post_nms_topk = int(pre_nms_topk), int(post_nms_topk)
        self.rpn_nms_thresh, self.min_box_size = float(rpn_nms_thresh), float(min_box_size)
        self.score_thresh, self.nms_thresh = float(score_thresh), float(nms_thresh)
        self.detections_per_image = int(detections_per_image)
        self.bbox_reg_weights = tuple(float(v) for v in bbox_reg_weights)
        # frames per pass through the heads: the box NMS scratch grows with frames x classes x proposals^2 / 8 bytes
        # (36 MB at 8 frames, 35 classes and 1000 proposals)
        self.frame_chunk = int(frame_chunk)

    def forward(self, images, bf16=False):
        with torch.no_grad():
            dev = _compute_device(images, self.pixel_mean)
            if images.dim() != 4 or images.shape[3] != 3:
                raise ValueError(f"images must be channels-last [T,H,W,3], got {tuple(images.shape)}")
            x = (_f32(images, dev) - _f32(self.pixel_mean, dev).view(1, 1, 1, 3)) / _f32(self.pixel_std, dev).view(1, 1, 1, 3)
            maps = self.backbone(x, bf16=bf16)
            t, h, w = images.shape[:3]
            sizes = torch.tensor([[float(h), float(w)]], dtype=torch.float32, device=dev).repeat(t, 1)
            return self.detect_from_maps(maps, sizes)

    def detect_from_maps(self, feature_maps, image_sizes):
        with torch.no_grad():
            dev = _compute_device(feature_maps, self.pixel_mean)
            bf16 = feature_maps.dtype == torch.bfloat16
            fm = feature_maps.to(dev).contiguous() if bf16 else _f32(feature_maps, dev)
            sizes = _f32(image_sizes, dev)
            if fm.dim() != 4 or tuple(sizes.shape) != (fm.shape[0], 2):
                raise ValueError(f"feature_maps [T,Hf,Wf,C] and image_sizes [T,2] expected, got {tuple(fm.shape)} and "
                                 f"{tuple(sizes.shape)}")
            cell = _f32(self.cell_anchors, dev)
            head, roi = self.proposal_generator.rpn_head, self.roi_heads
            out = []
            for lo in range(0, fm.shape[0], self.frame_chunk):
                f, s = fm[lo:lo + self.frame_chunk], sizes[lo:lo + self.frame_chunk].contiguous()
                logits, deltas = head(f)
                props, _, count = ops.rpn_proposals(logits, deltas, cell, self.stride, s, self.pre_nms_topk,
                                                    self.post_nms_topk, self.rpn_nms_thresh, self.min_box_size)
                # rows past `count` are zero boxes: they go through res5 as well and box_head_decode ignores them
                feats = roi(f, props.permute(1, 0, 2).contiguous())                     # [R, Tc, C]
                feats = feats.permute(1, 0, 2).float().contiguous()                     # [Tc, R, C]
                # one GEMM per frame: its split-K plan depends on the row count, a frame's logits must not depend on
                # how many frames share the call
                both = [roi.box_predictor(feats[i]) for i in range(feats.shape[0])]
                cls = torch.cat([b[0] for b in both])
                dl = torch.cat([b[1] for b in both])
                out.append(ops.box_detections(cls, dl, props, count, s, self.score_thresh, self.nms_thresh,
                                              self.detections_per_image, self.bbox_reg_weights))
            if not out:
                d = self.detections_per_image
                return (torch.zeros((0, d, 4), device=dev), torch.zeros((0, d), device=dev),
                        torch.zeros((0, d), dtype=torch.int64, device=dev), torch.zeros((0,), dtype=torch.int64, device=dev))
            return tuple(torch.cat([o[k] for o in out]) for k in range(4))
