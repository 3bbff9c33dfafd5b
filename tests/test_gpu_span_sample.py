"""The span anchor sampler on the GPU (csrc/spansample/tspn_span_sample.hip; ops.span_anchor_sample; the
RELPN.DPN.SPAN_LOSS.BATCH_SIZE_PER_SEGMENT path of DPN training) against the numpy restatement of
tests/span_sample_reference.py.

Everything the sampler computes is integer arithmetic, so mask and counts are compared exactly.  The case list lives in
tests/span_sample_reference.py; tests/test_span_sample_host.py checks, without a GPU, that it holds the sizes, key widths,
class mixes, quota regimes and threshold ties this file relies on.  The model test compares with the tolerances of
tests/test_gpu_span_loss.py's model test (losses rtol 2e-5, parameter gradients atol 2e-4 max|ref| + 1e-9)."""
import numpy as np
import pytest
import torch

import cases
import oracle
import sentinel_buffers as sb
import span_loss_reference as loss_ref
import span_sample_reference as ref
from train_reference import oracle_weights

pytestmark = pytest.mark.gpu


def key_of(tspn, case):
    return tspn.hashrng.stream_key(case["seed"], ref.tag_of(case))


def sample(tspn, device, label, case, **kw):
    """(mask, counts) of ops.span_anchor_sample as numpy arrays."""
    mask, counts = tspn.ops.span_anchor_sample(torch.from_numpy(np.array(label)).to(device), case["batch"], case["fraction"],
                                               key_of(tspn, case), case["key_bits"], **kw)
    return mask.cpu().numpy(), counts.cpu().numpy()


def check(got_mask, got_counts, mask, counts, what):
    assert got_mask.dtype == np.uint8 and got_mask.shape == mask.shape and got_counts.dtype == np.int64
    assert got_counts.tolist() == counts.tolist(), what
    diff = np.flatnonzero(got_mask.reshape(-1) != mask.reshape(-1))
    assert diff.size == 0, f"{what}: {diff.size} mask elements differ, first at {diff[:5].tolist()}"


@pytest.mark.parametrize("case_id", [c["id"] for c in ref.CASES])
def test_mask_and_counts_equal_the_restatement(tspn, device, case_id):
    case, label, mask, counts, _ = ref.reference(case_id)
    got_mask, got_counts = sample(tspn, device, label, case)
    check(got_mask, got_counts, mask, counts, case_id)


def test_threshold_decided_in_the_last_of_four_rounds(tspn, device):
    """Two negatives whose 32-bit keys agree in their upper 24 bits, the batch cut on the first of them."""
    case, label, mask, counts, info = ref.reference("last-round")
    assert info[1]["decided_round"] == 3
    check(*sample(tspn, device, label, case), mask, counts, "last-round")


def test_full_size_with_the_threshold_on_a_32_bit_tie(tspn, device):
    """A cfg2 segment's 595 200 anchors with 32-bit keys; the batch is cut between two negatives of EQUAL keys, so the
    lower flat index is in and the higher one out."""
    case, label, mask, counts, info = ref.reference("full-size-tie")
    lo, hi = info[1]["equal"].tolist()
    assert case["n"] == 595200 and case["key_bits"] == 32 and mask[lo] == 1 and mask[hi] == 0
    got_mask, got_counts = sample(tspn, device, label, case)
    assert (got_mask[lo], got_mask[hi]) == (1, 0)
    check(got_mask, got_counts, mask, counts, "full-size-tie")
    # as [P, A, T] labels the mask keeps the shape
    shaped = label.reshape(992, 4, 150)
    got_mask, _ = sample(tspn, device, shaped, case)
    assert got_mask.shape == (992, 4, 150) and np.array_equal(got_mask.reshape(-1), mask)


# ------------------------------------------------------------------------------------------- guarded outputs
MASK_FILL, COUNT_FILL, WORD_FILL = 0xAB, -77, 0x5A5A5A5A


def _held(n, device, dtype, fill, offset=0):
    """(buffer, view): a buffer of `fill` and a view of n elements sb.GUARD + offset elements into it."""
    buf = torch.full((n + 2 * sb.GUARD + offset,), fill, dtype=dtype, device=device)
    return buf, buf[sb.GUARD + offset:sb.GUARD + offset + n]


def _written_inside_only(buf, v, fill, what):
    b = buf.cpu()
    n, lo = v.numel(), v.storage_offset()
    assert bool((b[:lo] == fill).all()) and bool((b[lo + n:] == fill).all()), f"{what}: wrote outside the output"
    never = int((b[lo:lo + n] == fill).sum())
    assert never == 0, f"{what}: {never} of {n} elements never written"


def _launch_held(tspn, device, label, case, offset):
    """The entry through the C ABI on guarded buffers; returns the buffers and views."""
    lib, p = tspn._abi.lib(), sb.p
    n = label.size
    lab_buf, lab = _held(n, device, torch.int8, 0, offset)
    lab.copy_(torch.from_numpy(np.array(label)))
    mask_buf, mask = _held(n, device, torch.uint8, MASK_FILL, offset)
    cnt_buf, cnt = _held(4, device, torch.int64, COUNT_FILL)
    words = lib.tspn_span_anchor_sample_partials(n)
    par_buf, par = _held(words, device, torch.int32, WORD_FILL)
    rc = lib.tspn_span_anchor_sample(p(lab), n, key_of(tspn, case), case["key_bits"], case["batch"], ref.want_pos_of(case),
                                     p(par), p(cnt), p(mask), tspn.ops._stream())
    assert rc == 0, lib.tspn_last_error().decode()
    return (mask_buf, mask), (cnt_buf, cnt), (par_buf, par)


@pytest.mark.parametrize("offset", [0, 3], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("case_id", ["n65-k4-mixed-b256-f0.5", "n12293-k4-mixed-b256-f0.5", "n12293-k32-mixed-b256-f0.5"])
def test_sentinels_and_unaligned_operands(tspn, device, case_id, offset):
    """mask, counts and partials inside guarded buffers: nothing outside is written, every element inside is (a mask
    element is 0 or 1, a count is >= 0, a histogram bin, an offset or a state word never reaches 0x5A5A5A5A on these
    sizes).  Offset 0 takes the 16-byte label loads and mask stores, offset 3 the byte forms."""
    case, label, mask, counts, _ = ref.reference(case_id)
    (mask_buf, m), (cnt_buf, c), (par_buf, par) = _launch_held(tspn, device, label, case, offset)
    assert (m.data_ptr() % 16 == 0) == (offset == 0)
    _written_inside_only(mask_buf, m, MASK_FILL, "mask")
    _written_inside_only(cnt_buf, c, COUNT_FILL, "counts")
    _written_inside_only(par_buf, par, WORD_FILL, "partials")
    check(m.cpu().numpy(), c.cpu().numpy(), mask, counts, f"{case_id} held at offset {offset}")
    # the state ends with the quotas and the sizes of both classes
    words = par.cpu().numpy().view(np.uint32)
    assert words[4:8].tolist() == [counts[2], counts[3], counts[0], counts[1]]


def test_stale_outputs_do_not_change_the_result(tspn, device):
    """A second launch whose partials, counts and mask hold garbage gives the bits of the first, partials included."""
    for case_id in ("n12293-k17-mixed-b256-f0.5", "n1052675-k4-mixed-b256-f0.5"):
        case, label, mask, counts, _ = ref.reference(case_id)
        lib, p = tspn._abi.lib(), sb.p
        n = label.size
        lab = torch.from_numpy(np.array(label)).to(device)
        words = lib.tspn_span_anchor_sample_partials(n)
        results = []
        for fill in (None, "garbage"):
            g = torch.Generator(device="cpu").manual_seed(5)
            if fill is None:
                m = torch.zeros(n, dtype=torch.uint8, device=device)
                c = torch.zeros(4, dtype=torch.int64, device=device)
                par = torch.zeros(words, dtype=torch.int32, device=device)
            else:
                m = torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g).to(device)
                c = torch.randint(-2 ** 62, 2 ** 62, (4,), dtype=torch.int64, generator=g).to(device)
                par = torch.randint(-2 ** 31, 2 ** 31 - 1, (words,), dtype=torch.int32, generator=g).to(device)
            rc = lib.tspn_span_anchor_sample(p(lab), n, key_of(tspn, case), case["key_bits"], case["batch"],
                                             ref.want_pos_of(case), p(par), p(c), p(m), tspn.ops._stream())
            assert rc == 0
            results.append((m.cpu().numpy(), c.cpu().numpy(), par.cpu().numpy()))
        for a, b in zip(*results):
            assert np.array_equal(a, b), case_id
        check(results[1][0], results[1][1], mask, counts, case_id)


def test_two_stream_keys_give_two_masks_with_equal_counts(tspn, device):
    case, label, mask, counts, _ = ref.reference("n12293-k32-mixed-b256-f0.5")
    lab = torch.from_numpy(np.array(label)).to(device)
    k0, k1 = (tspn.hashrng.stream_key(9, f"span_sample/{c}") for c in (0, 1))
    assert k0 != k1
    m0, c0 = tspn.ops.span_anchor_sample(lab, 256, 0.5, k0)
    m1, c1 = tspn.ops.span_anchor_sample(lab, 256, 0.5, k1)
    assert c0.cpu().tolist() == c1.cpu().tolist() == counts.tolist()
    assert int(m0.sum()) == int(m1.sum()) == 256 and not torch.equal(m0, m1)
    for tag, got in (("span_sample/0", m0), ("span_sample/1", m1)):
        want, _, _ = ref.sample_ref(label, 9, tag, 32, 256, 128)
        assert np.array_equal(got.cpu().numpy(), want), tag
    # the same key again: the same mask
    assert torch.equal(tspn.ops.span_anchor_sample(lab, 256, 0.5, k0)[0], m0)


def test_refusals_and_the_empty_case(tspn, device):
    case, label, mask, counts, _ = ref.reference("n65-k4-mixed-b256-f0.5")
    A_, lib, p = tspn._abi, tspn._abi.lib(), sb.p
    n = label.size
    lab = torch.from_numpy(np.array(label)).to(device)
    mask_buf, m = _held(n, device, torch.uint8, MASK_FILL)
    cnt_buf, c = _held(4, device, torch.int64, COUNT_FILL)
    par_buf, par = _held(lib.tspn_span_anchor_sample_partials(n), device, torch.int32, WORD_FILL)
    stream = tspn.ops._stream()

    def call(label_=lab, n_=n, key_bits=32, batch=256, want_pos=128, partials=par, counts_=c, mask_=m):
        return lib.tspn_span_anchor_sample(p(label_), n_, 1, key_bits, batch, want_pos, p(partials), p(counts_), p(mask_), stream)

    for kw in ("label_", "partials", "counts_", "mask_"):
        assert call(**{kw: None}) == A_.TSPN_EINVAL, kw
    assert call(n_=-1) == A_.TSPN_EINVAL and call(n_=2 ** 31) == A_.TSPN_EUNSUPPORTED
    assert call(key_bits=0) == A_.TSPN_EINVAL and call(key_bits=33) == A_.TSPN_EINVAL
    assert call(batch=-1, want_pos=0) == A_.TSPN_EINVAL
    assert call(want_pos=-1) == A_.TSPN_EINVAL and call(want_pos=257) == A_.TSPN_EINVAL
    torch.cuda.synchronize(device)
    for buf, fill in ((mask_buf, MASK_FILL), (cnt_buf, COUNT_FILL), (par_buf, WORD_FILL)):
        assert bool((buf == fill).all()), "a refused call wrote to an output"
    # n = 0: counts = 0, nothing else is touched (label, partials and mask may be null)
    assert lib.tspn_span_anchor_sample(None, 0, 1, 32, 256, 128, None, p(c), None, stream) == A_.TSPN_OK
    _written_inside_only(cnt_buf, c, COUNT_FILL, "counts of n = 0")
    assert c.cpu().tolist() == [0, 0, 0, 0]
    m0, c0 = tspn.ops.span_anchor_sample(torch.zeros((0, 4, 7), dtype=torch.int8, device=device), 256, 0.5, 1)
    assert m0.shape == (0, 4, 7) and m0.dtype == torch.uint8 and c0.cpu().tolist() == [0, 0, 0, 0]
    # batch = 0 is served: the class sizes, and a mask of zeros
    m1, c1 = tspn.ops.span_anchor_sample(lab, 0, 0.5, 1)
    assert c1.cpu().tolist() == [counts[0], counts[1], 0, 0] and not bool(m1.any())
    # the op's own checks
    ops = tspn.ops
    with pytest.raises(TypeError):
        ops.span_anchor_sample(lab.int(), 256, 0.5, 1)
    with pytest.raises(ValueError):
        ops.span_anchor_sample(lab, -1, 0.5, 1)
    with pytest.raises(ValueError):
        ops.span_anchor_sample(lab, 256, 1.5, 1)
    with pytest.raises(ValueError):
        ops.span_anchor_sample(lab, 256, 0.5, 1, mask=torch.empty(n + 1, dtype=torch.uint8, device=device))
    with pytest.raises(tspn._abi.TspnError):
        ops.span_anchor_sample(lab, 256, 0.5, 1, key_bits=0)
    # a mask passed in is the mask returned; a non-contiguous label is taken in its logical order
    out = torch.empty(n, dtype=torch.uint8, device=device)
    got, _ = ops.span_anchor_sample(lab, case["batch"], case["fraction"], key_of(tspn, case), case["key_bits"], mask=out)
    assert got is out and np.array_equal(out.cpu().numpy(), mask)
    two = torch.stack([lab, lab], dim=1)[:, 0]
    assert not two.is_contiguous()
    got, _ = ops.span_anchor_sample(two, case["batch"], case["fraction"], key_of(tspn, case), case["key_bits"])
    assert np.array_equal(got.cpu().numpy(), mask)


# ------------------------------------------------------------------------------------------------------- the model
BATCH, SEED = 64, 11


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _model(tspn, device, D, **extra):
    cfg = cases.baseline_cfg(**{"RELPN.USE_PPN": False, "RELPN.USE_DPN": True, "RELPN.DPN.IN_CHANNELS": 2 * D,
                                "PREDICT.FEATURE_DIM": 2 * D, **extra})
    sd = tspn.synth.make_weights(3, c=2 * D, bias_std=0.05)
    model = tspn.BaseModel(cfg)
    own = model.state_dict()
    model.load_state_dict({k: _t(v) for k, v in sd.items() if k in own})
    return model.to(device).train(), sd


def _segments(tspn, device, form):
    """The two segments of tests/test_gpu_span_loss.py's model test (N = 5 and 6, T = 30, D = 16, G = 3)."""
    D, T, G, K = 16, 30, 3, 132
    segments, plists, tlists = [], [], []
    for i, N in enumerate((5, 6)):
        v = tspn.synth.make_video(95 + i, N, T, D)
        pairs = oracle.pair_index(N)
        P = pairs.shape[0]
        gt = loss_ref.make_gt(70 + i, P, G, T)
        targets = _t((tspn.hashrng.uniform(96 + i, "tg", (P, K)) < 0.05).astype(np.float32))
        if form == "tracklets":
            plist = tspn.PairList.from_tracklets(_t(v["tracklet_feats"]), _t(v["tracklet_boxes"]), _t(v["track_cls_logits"]))
        else:
            plist = tspn.PairList(oracle.pair_gather(_t(v["tracklet_feats"]), _t(v["tracklet_boxes"]), pairs)[0])
        tlist = tspn.TargetList(targets)
        tlist.add_field("spans", _t(gt))
        segments.append((v, pairs, gt, targets))
        plists.append(plist.to(device))
        tlists.append(tlist.to(device))
    return segments, plists, tlists


def _dpn_grads(model):
    h = model.relpn.duration_proposal_network.dpn_head
    return {"conv_w": h.conv.weight.grad, "conv_b": h.conv.bias.grad, "dur_w": h.duration_pred.weight.grad,
            "dur_b": h.duration_pred.bias.grad, "rel_w": h.relness_pred.weight.grad, "rel_b": h.relness_pred.bias.grad}


def _sampled_reference(segments, sd, sizes, first):
    """Float64 restatement of one training step with sampling on: span_loss_reference's step, each segment's losses under
    the restatement's mask for stream (SEED, "span_sample/{first + segment}").  Returns losses, parameter gradients and
    the masks' counts."""
    w = {k: x.double().requires_grad_(True) for k, x in oracle_weights(sd).items()}
    losses, all_counts = {"loss_relationness": 0, "loss_duration_proposal": 0}, []
    for c, (v, pairs, gt, _) in enumerate(segments):
        pf, _ = oracle.pair_gather(_t(v["tracklet_feats"]), _t(v["tracklet_boxes"]), pairs)
        rel, dur, _ = oracle.dpn_head(pf.double(), w["conv_w"], w["conv_b"], w["dur_w"], w["dur_b"], w["rel_w"], w["rel_b"])
        heads = torch.cat([rel, dur], dim=1)
        T = heads.shape[2]
        label, matched, _ = loss_ref.labels_ref(gt, sizes(T), T)
        mask, counts, _ = ref.sample_ref(label, SEED, f"span_sample/{first + c}", 32, BATCH, BATCH // 2)
        lr, lp, n_lab, n_pos = loss_ref.losses_torch(heads, gt, sizes(T), label, matched, mask, loss_ref.BETA)
        assert n_lab == counts[2] + counts[3] == BATCH and n_pos == counts[2]
        # the same numbers from span_loss_ref on the restated heads rounded to fp32, as a check of this function
        out = loss_ref.span_loss_ref(heads.detach().float().numpy(), gt, sizes(T), mask=mask)[0]
        np.testing.assert_allclose([float(lr.detach()), float(lp.detach())], out[:2], rtol=1e-5)
        losses["loss_relationness"] = losses["loss_relationness"] + lr
        losses["loss_duration_proposal"] = losses["loss_duration_proposal"] + lp
        all_counts.append(counts)
    sum(losses.values()).backward()
    return {k: float(x.detach()) for k, x in losses.items()}, {k: x.grad for k, x in w.items()}, all_counts


@pytest.mark.parametrize("form", ["tracklets", "dense"])
def test_model_samples_a_balanced_mini_batch_per_segment(tspn, device, form):
    """BATCH_SIZE_PER_SEGMENT = 64 on the two segments of the span-loss model test, two successive steps: segment c of
    step s draws stream (SAMPLE_SEED, "span_sample/{2 s + c}").  The span losses and the DPN-head parameter gradients of
    each step against the float64 restatement under the restatement's masks; after reseed_span_sampler the first step
    repeats bit for bit."""
    model, sd = _model(tspn, device, 16, **{"RELPN.DPN.SPAN_LOSS.BATCH_SIZE_PER_SEGMENT": BATCH,
                                           "RELPN.DPN.SPAN_LOSS.SAMPLE_SEED": SEED})
    dpn = model.relpn.duration_proposal_network
    assert (dpn.span_batch, dpn.span_positive_fraction, dpn._span_sample_count) == (BATCH, 0.5, 0)
    assert not any("span_sample" in k for k in model.state_dict())
    segments, plists, tlists = _segments(tspn, device, form)
    steps = []
    for step in range(2):
        model.zero_grad(set_to_none=True)
        loss = model(plists, tlists)
        assert set(loss) == {"loss_relationness", "loss_duration_proposal", "loss_rel"}
        (loss["loss_relationness"] + loss["loss_duration_proposal"]).backward()
        assert dpn._span_sample_count == 2 * (step + 1)
        ref_loss, ref_grad, counts = _sampled_reference(segments, sd, model.anchor_sizes, 2 * step)
        assert all(c[0] > BATCH // 2 and c[1] > BATCH // 2 for c in counts)     # both quotas bind: the sample is balanced
        print(step, {k: (loss[k].item(), ref_loss[k]) for k in ref_loss})
        for k in ref_loss:
            np.testing.assert_allclose(loss[k].item(), ref_loss[k], rtol=2e-5, err_msg=f"step {step}: {k}")
        for k, gq in _dpn_grads(model).items():
            r = ref_grad[k].numpy()
            assert np.abs(r).max() > 0, k
            np.testing.assert_allclose(gq.cpu().numpy(), r, rtol=0, atol=2e-4 * np.abs(r).max() + 1e-9,
                                       err_msg=f"step {step}: {k}")
        steps.append({k: loss[k].detach().cpu().numpy().copy() for k in ref_loss})
    # the counter advanced: the second step saw other masks on the same weights and inputs
    assert steps[0]["loss_relationness"] != steps[1]["loss_relationness"]
    dpn.reseed_span_sampler(SEED)
    again = model(plists, tlists)
    for k in steps[0]:
        assert again[k].detach().cpu().numpy().tobytes() == steps[0][k].tobytes(), k
    dpn.reseed_span_sampler(SEED, start=2)
    again = model(plists, tlists)
    for k in steps[1]:
        assert again[k].detach().cpu().numpy().tobytes() == steps[1][k].tobytes(), k


def test_model_without_sampling_is_the_three_entries(tspn, device):
    """The default config (BATCH_SIZE_PER_SEGMENT = 0): the model's span losses are bit-equal to a direct call of the
    labelling and loss entries on its heads, and no sampler stream is drawn."""
    model, _ = _model(tspn, device, 16)
    dpn = model.relpn.duration_proposal_network
    assert dpn.span_batch == 0 and dpn._next_span_sample() is None
    _, plists, tlists = _segments(tspn, device, "tracklets")
    loss = model(plists, tlists)
    assert dpn._span_sample_count == 0
    want = {"loss_relationness": 0, "loss_duration_proposal": 0}
    with torch.no_grad():
        for plist, tlist in zip(plists, tlists):
            heads = dpn._train_heads(plist).contiguous()
            gt = tlist.get_field("spans").contiguous()
            sizes = dpn.anchor_sizes(heads.shape[2])
            label, matched = tspn.ops.span_anchor_labels(gt, sizes, heads.shape[2], dpn.span_pos_iou, dpn.span_neg_iou)
            out, _ = tspn.ops.span_loss(heads, gt, sizes, label, matched, beta=dpn.span_beta)
            want["loss_relationness"] = want["loss_relationness"] + out[0].float()
            want["loss_duration_proposal"] = want["loss_duration_proposal"] + out[1].float()
    for k, v in want.items():
        assert loss[k].detach().cpu().numpy().tobytes() == v.cpu().numpy().tobytes(), k
