"""float64 restatement of the detector's two small modules and of its pixel normalisation, with the error envelopes
the device is held to (DESIGN.md 3 "Detector module bounds").  torch on the CPU, no device.

`rpn_head` is detectron2 v0.6's StandardRPNHead and `box_predictor` the two linear layers of FastRCNNOutputLayers, from
the SEPARATE weights of a state dict (`conv.*`, `objectness_logits.*`, `anchor_deltas.*`; `cls_score.*`, `bbox_pred.*`)
as torch.nn.functional.conv2d and `@` take them: nothing is concatenated or padded here, which is what detector.py does
and what the tests compare against this file.

The bounds are computed, per output element, from the operands: for an fp32 dot product of n terms plus a bias, summed
in ANY order (any tiling, any split-K plan), |fp32 - float64| <= (n + 2) u (sum |w||x| + |b|), u = 2^-24."""
import torch
import torch.nn.functional as F

from oracle import roi_head_oracle as ro

U = 2.0 ** -24            # fp32 unit roundoff
H16 = 2.0 ** -8           # bf16 unit roundoff: half an ulp, relative


def _nchw(x_nhwc):
    return x_nhwc.permute(0, 3, 1, 2).double()


def _nhwc(y_nchw):
    return y_nchw.permute(0, 2, 3, 1).contiguous()


def _r16(x):
    return x.float().to(torch.bfloat16).double()


def _d(sd, key):
    v = sd[key]
    return (v if isinstance(v, torch.Tensor) else torch.as_tensor(v)).detach().cpu().double()


def rpn_head_with_bounds(x_nhwc, sd, dtype=torch.float32):
    """x [T,H,W,C] -> dict of channels-last float64 tensors:
    `logits` [T,H,W,A], `deltas` [T,H,W,4A] (channel 4a + k, the conv's own order): the module's result (for
    torch.bfloat16 rounded to bf16 once, as the device's is);
    `raw_logits`, `raw_deltas`: the same before that last rounding (equal to the above for fp32);
    `logits_bound`, `deltas_bound`: the envelope of |device - raw| per element."""
    bf16 = dtype == torch.bfloat16
    w1, b1 = _d(sd, "conv.weight"), _d(sd, "conv.bias")
    heads = [(_d(sd, "objectness_logits.weight"), _d(sd, "objectness_logits.bias")),
             (_d(sd, "anchor_deltas.weight"), _d(sd, "anchor_deltas.bias"))]
    x = _nchw(x_nhwc.detach().cpu())
    n1, n2 = 9 * w1.shape[1], w1.shape[0]
    if bf16:
        t = ro.conv2d_bf16(x, w1, b1, padding=1, relu=True)               # bf16 operands, t rounded to bf16 once
        x, w1 = _r16(x), _r16(w1)
    else:
        t = F.relu(F.conv2d(x, w1, b1, padding=1))
    # e1: the device's 3x3 sum against float64, before the ReLU (1-Lipschitz, so after it as well)
    e1 = (n1 + 2) * U * (F.conv2d(x.abs(), w1.abs(), b1.abs(), padding=1))
    if bf16:
        # rounding to bf16 is monotone and moves v by at most 2^-8 |v|: device and reference t differ by at most
        # e1 (1 + 2^-8) + 2^-7 t / (1 - 2^-8) -- e1 plus one bf16 ulp of t
        e1 = e1 * (1 + H16) + 2 * H16 * t / (1 - H16)
    out = {}
    for name, (w2, b2) in zip(("logits", "deltas"), heads):
        if bf16:
            raw = F.conv2d(t, _r16(w2), b2)
            w2 = _r16(w2)
            val = _r16(raw)
        else:
            raw = val = F.conv2d(t, w2, b2)
        e2 = (n2 + 2) * U * F.conv2d(t.abs(), w2.abs(), b2.abs()) + F.conv2d(e1, w2.abs())
        if bf16:
            e2 = e2 * (1 + H16) + H16 * raw.abs()                         # half a bf16 ulp of the device's own sum
        out[name], out["raw_" + name], out[name + "_bound"] = _nhwc(val), _nhwc(raw), _nhwc(e2)
    return out


def rpn_head(x_nhwc, sd, dtype=torch.float32):
    """-> (objectness logits [T,H,W,A], anchor deltas [T,H,W,4A]) in float64."""
    r = rpn_head_with_bounds(x_nhwc, sd, dtype)
    return r["logits"], r["deltas"]


def box_predictor_with_bounds(x, sd):
    """x [R,C] -> (cls_logits [R,K+1], deltas [R,4K], and the envelope of |device - float64| of each), float64."""
    x = x.detach().cpu().double()
    out, bounds = [], []
    for name in ("cls_score", "bbox_pred"):
        w, b = _d(sd, name + ".weight"), _d(sd, name + ".bias")
        out.append(x @ w.T + b)
        bounds.append((w.shape[1] + 2) * U * (x.abs() @ w.abs().T + b.abs()))
    return out[0], out[1], bounds[0], bounds[1]


def box_predictor(x, sd):
    """-> (x @ cls_score.weight.T + bias, x @ bbox_pred.weight.T + bias) in float64, as two products."""
    return box_predictor_with_bounds(x, sd)[:2]


def pixel_normalise(images, mean, std):
    """(images [T,H,W,3] - mean[c]) / std[c] in float64, mean and std read as the fp32 values the module holds."""
    m = torch.as_tensor(mean, dtype=torch.float32).double().view(1, 1, 1, -1)
    s = torch.as_tensor(std, dtype=torch.float32).double().view(1, 1, 1, -1)
    return (images.detach().cpu().double() - m) / s


# ------------------------------------------------------------------------------------ seeded weights and exact cases
RPN_ANCHORS = (3, 7, 15, 32)                      # 5A = 15, 35, 75, 160: padded to 32, to 64, to 96, not at all
RPN_MAPS = ((1, 1, 1), (2, 5, 7), (3, 9, 13))     # [T,H,W]
RPN_WIDE = (1024, 15, (2, 5, 7))                  # the detector's own width, once
PREDICTOR_SHAPES = [(r, c, k) for r in (1, 65, 300, 1000) for c in (64, 2048) for k in (1, 35)]


def rpn_weights(hashrng, seed, channels, anchors, delta_gain=1.0, size_bias=0.0):
    """Seeded StandardRPNHead state dict: every bias non-zero, every row distinct.  `delta_gain` scales the delta
    weights and `size_bias` is added to the biases of the dw / dh channels (4a + 2, 4a + 3): larger boxes, which the
    clip and the NMS merge into fewer proposals."""
    t = torch.from_numpy
    c, a = channels, anchors
    sd = {"conv.weight": t(hashrng.normal(seed, "rpn.conv.w", (c, c, 3, 3), std=(2.0 / (9 * c)) ** 0.5)),
            "conv.bias": t(hashrng.uniform(seed, "rpn.conv.b", (c,), -0.3, 0.3)),
            "objectness_logits.weight": t(hashrng.normal(seed, "rpn.obj.w", (a, c, 1, 1), std=(4.0 / c) ** 0.5)),
            "objectness_logits.bias": t(hashrng.uniform(seed, "rpn.obj.b", (a,), -0.5, 0.5)),
            "anchor_deltas.weight": t(hashrng.normal(seed, "rpn.dl.w", (4 * a, c, 1, 1), std=(1.0 / c) ** 0.5)),
            "anchor_deltas.bias": t(hashrng.uniform(seed, "rpn.dl.b", (4 * a,), -0.2, 0.2))}
    sd["anchor_deltas.weight"] = sd["anchor_deltas.weight"] * delta_gain
    sd["anchor_deltas.bias"][2::4] += size_bias
    sd["anchor_deltas.bias"][3::4] += size_bias
    return sd


def predictor_weights(hashrng, seed, channels, classes):
    t = torch.from_numpy
    c, k = channels, classes
    return {"cls_score.weight": t(hashrng.normal(seed, "cls.w", (k + 1, c), std=(4.0 / c) ** 0.5)),
            "cls_score.bias": t(hashrng.uniform(seed, "cls.b", (k + 1,), -0.5, 0.5)),
            "bbox_pred.weight": t(hashrng.normal(seed, "box.w", (4 * k, c), std=(1.0 / c) ** 0.5)),
            "bbox_pred.bias": t(hashrng.uniform(seed, "box.b", (4 * k,), -0.5, 0.5))}


def rpn_exact_case(channels, anchors, shape):
    """Integers all the way: a centre-tap identity `conv` with integer biases (some negative, so the ReLU cuts), one-hot
    head rows with small integer weights that pick distinct input channels, distinct integer head biases, a non-negative
    integer map.  -> (x fp32 [T,H,W,C], state dict, logits [T,H,W,A], deltas [T,H,W,4A]) with the two results worked
    out by indexing, without a convolution.  Needs 5 A <= channels and channels coprime to 11."""
    c, a = channels, anchors
    assert 5 * a <= c and c % 11
    n = shape[0] * shape[1] * shape[2]
    x = ((torch.arange(n * c, dtype=torch.float64) * 7) % 23).reshape(*shape, c)
    cb = (torch.arange(c, dtype=torch.float64) % 9) - 6                   # -6 .. 2
    w1 = torch.zeros((c, c, 3, 3), dtype=torch.float64)
    w1[torch.arange(c), torch.arange(c), 1, 1] = 1
    t = torch.clamp(x + cb, min=0)
    rows = torch.arange(5 * a)
    pick = (rows * 11 + 3) % c                                            # distinct: 11 is coprime to c
    wv = (rows % 3 + 1).double() * torch.where(rows % 2 == 0, 1.0, -1.0)  # +-1, +-2, +-3
    hb = rows.double() + 1                                                 # |y| <= 72 + 160: bf16 integers
    y = t[..., pick] * wv + hb
    w2 = torch.zeros((5 * a, c, 1, 1), dtype=torch.float64)
    w2[rows, pick, 0, 0] = wv
    sd = {"conv.weight": w1.float(), "conv.bias": cb.float(),
          "objectness_logits.weight": w2[:a].float(), "objectness_logits.bias": hb[:a].float(),
          "anchor_deltas.weight": w2[a:].float(), "anchor_deltas.bias": hb[a:].float()}
    return x.float(), sd, y[..., :a].contiguous(), y[..., a:].contiguous()


def predictor_exact_case(rows, channels, classes):
    """One-hot integer weights, distinct integer biases, integer features -> (x fp32 [R,C], state dict, cls [R,K+1],
    deltas [R,4K]) worked out by indexing."""
    r, c, k = rows, channels, classes
    x = (((torch.arange(r * c, dtype=torch.float64) * 5) % 31) - 15).reshape(r, c)
    out = torch.arange(5 * k + 1)
    pick = (out * 11 + 5) % c
    wv = (out % 4 + 1).double() * torch.where(out % 2 == 0, 1.0, -1.0)
    b = 50.0 - out.double() * 2
    w = torch.zeros((5 * k + 1, c), dtype=torch.float64)
    w[out, pick] = wv
    y = x[:, pick] * wv + b
    sd = {"cls_score.weight": w[:k + 1].float(), "cls_score.bias": b[:k + 1].float(),
          "bbox_pred.weight": w[k + 1:].float(), "bbox_pred.bias": b[k + 1:].float()}
    return x.float(), sd, y[:, :k + 1].contiguous(), y[:, k + 1:].contiguous()
