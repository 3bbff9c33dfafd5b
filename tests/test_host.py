"""Host-side logic that needs no GPU: config surface, container types, state_dict contract,
the C-ABI library's exports and error paths, and the no-CPU-fallback rule."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cases

EXPECTED_KEYS = {
    "relpn.pair_proposal_network.ppn_head.sub_emb.0.weight": (64, 35),
    "relpn.pair_proposal_network.ppn_head.sub_emb.0.bias": (64,),
    "relpn.pair_proposal_network.ppn_head.sub_emb.2.weight": (35, 64),
    "relpn.pair_proposal_network.ppn_head.sub_emb.2.bias": (35,),
    "relpn.pair_proposal_network.ppn_head.obj_emb.0.weight": (64, 35),
    "relpn.pair_proposal_network.ppn_head.obj_emb.0.bias": (64,),
    "relpn.pair_proposal_network.ppn_head.obj_emb.2.weight": (35, 64),
    "relpn.pair_proposal_network.ppn_head.obj_emb.2.bias": (35,),
    "relpn.duration_proposal_network.dpn_head.conv.weight": (1024, 1024, 3),
    "relpn.duration_proposal_network.dpn_head.conv.bias": (1024,),
    "relpn.duration_proposal_network.dpn_head.duration_pred.weight": (8, 1024, 1),
    "relpn.duration_proposal_network.dpn_head.duration_pred.bias": (8,),
    "classifier.rel_predictor.weight": (132, 11070),
    "classifier.rel_predictor.bias": (132,),
}  # SURVEY.md §8b (probed from the reference's BaseModel.state_dict())


def test_config_defaults_and_yaml_overlay(tspn, tmp_path):
    cfg = tspn.default_cfg()
    assert cfg.RELPN.USE_PPN is True and cfg.RELPN.USE_DPN is True  # defaults.py:52,61
    assert cfg.PREDICT.FEATURE_DIM == 11070 and cfg.PREDICT.PREDICATE_NUM == 132
    assert cfg.RELPN.DPN.IN_CHANNELS == 1024 and cfg.RELPN.DPN.NUM_ANCHORS_PER_LOCATION == 4
    y = tmp_path / "baseline.yaml"
    y.write_text("RELPN:\n  USE_PPN: False\n  USE_DPN: False\n  PPN:\n    POSITIVE_FRACTION: 0.25\n"
                 "PREDICT:\n  TOPK_PER_SEG: 200\nSOLVER:\n  BASE_LR: 1e-2\n")
    cfg = tspn.load_cfg(str(y), **{"RELPN.DPN.IN_CHANNELS": 64})
    assert cfg.RELPN.USE_PPN is False and cfg.RELPN.PPN.POSITIVE_FRACTION == 0.25
    assert cfg.RELPN.PPN.NUM_PAIR_PROPOSALS == 256  # untouched default survives the overlay
    assert cfg.RELPN.DPN.IN_CHANNELS == 64 and cfg.SOLVER.BASE_LR == "1e-2"
    with pytest.raises(AttributeError):
        cfg.RELPN.NOPE
    (tmp_path / "evil.yaml").write_text("!!python/object/new:os.system [echo]\n")
    with pytest.raises(Exception):  # safe_load refuses python tags (cf. configs/baseline_config.yaml)
        tspn.load_cfg(str(tmp_path / "evil.yaml"))


def test_state_dict_contract(tspn):
    model = tspn.BaseModel(cases.baseline_cfg())
    sd = model.state_dict()
    for k, shape in EXPECTED_KEYS.items():
        assert k in sd and tuple(sd[k].shape) == shape, k
    extra = set(sd) - set(EXPECTED_KEYS)
    assert extra == {"relpn.duration_proposal_network.dpn_head.relness_pred.weight",
                     "relpn.duration_proposal_network.dpn_head.relness_pred.bias"}
    # a reference checkpoint (no relness_pred, DDP 'module.' prefix stripped by serialize.py:13-16)
    ref_ckpt = {k: torch.full_like(v, 0.5) for k, v in sd.items() if k in EXPECTED_KEYS}
    model.load_state_dict(ref_ckpt)  # strict=True must accept it
    assert float(model.classifier.rel_predictor.weight[0, 0]) == 0.5
    with pytest.raises(RuntimeError):
        model.load_state_dict({k: v for k, v in ref_ckpt.items() if "classifier" not in k})
    # initialisers: N(0, 0.01^2) / zero bias (model.py:81-83, dpn.py:65-67)
    fresh = tspn.BaseModel(cases.baseline_cfg())
    w = fresh.classifier.rel_predictor.weight
    assert abs(float(w.std()) - 0.01) < 5e-4 and float(fresh.classifier.rel_predictor.bias.abs().max()) == 0
    assert float(fresh.relpn.duration_proposal_network.dpn_head.conv.bias.abs().max()) == 0


def test_pair_list_semantics(tspn):
    feats = torch.arange(12.0).reshape(4, 3)
    pl = tspn.PairList(feats)
    pl.add_field("track_cls_logits", torch.ones(2, 35))
    pl.add_field("tracklet_pairs", np.array([[0, 1], [1, 0], [0, 1], [1, 0]]))
    pl.add_field("num_tracklets", np.int64(2))
    assert len(pl) == 4 and pl.has_field("tracklet_pairs") and not pl.has_field("x")
    assert pl.fields() == ["track_cls_logits", "tracklet_pairs", "num_tracklets"]
    moved = pl.to("cpu")
    assert isinstance(moved, tspn.PairList) and moved is not pl
    assert isinstance(moved.get_field("tracklet_pairs"), np.ndarray)  # numpy fields stay on the host
    sub = tspn.PairList(feats)
    sub.add_field("tracklet_pairs", np.array([[0, 1], [1, 0], [0, 1], [1, 0]]))
    sl = sub[1:3]
    assert len(sl) == 2 and sl.get_field("tracklet_pairs").shape == (2, 2)
    only = pl.copy_with_fields("num_tracklets")
    assert only.fields() == ["num_tracklets"]
    with pytest.raises(KeyError):
        pl.copy_with_fields(["missing"])
    assert pl.copy_with_fields(["missing"], skip_missing=True).fields() == []
    assert repr(pl) == "PairList(num_feats=4)"
    tl = tspn.TargetList(torch.zeros(4, 132))
    assert len(tl) == 4 and repr(tl) == "TargetList(num_targets=4)"
    tr = tspn.PairList.from_tracklets(torch.zeros(5, 30, 8))
    assert len(tr) == 20 and tr.get_field("num_tracklets") == 5 and tr.features.shape == (20, 0)


def test_abi_library_exports_every_declared_symbol(tspn):
    names = tspn._abi.header_symbols()
    assert len(names) >= 19 and "tspn_forward_fused_f32" in names
    assert set(names) == set(tspn._abi.PROTOTYPES), "ctypes prototypes out of sync with include/tspn_mi355x.h"
    assert os.path.exists(tspn._abi.LIB_PATH), "libtspn_mi355x.so not built (run __graft_entry__.build())"
    raw = ctypes.CDLL(tspn._abi.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"library does not export {n}"
    lib = tspn._abi.lib()
    assert lib.tspn_version() == tspn._abi.ABI_VERSION == 7
    assert lib.tspn_fused_desc_size() == ctypes.sizeof(tspn._abi.FusedDesc)
    assert lib.tspn_fused_bf16_desc_size() == ctypes.sizeof(tspn._abi.FusedBf16Desc)
    assert lib.tspn_error_string(-3) == b"workspace too small"


def test_abi_argument_validation_without_gpu(tspn):
    """Argument checks return before any HIP call, so they run on a GPU-less host."""
    lib = tspn._abi.lib()
    rc = lib.tspn_predicate_head_f32(None, 4, 8, 8, None, None, 2, None, 1, None, 0, None)
    assert rc == tspn._abi.TSPN_EINVAL and b"null pointer" in lib.tspn_last_error()
    with pytest.raises(tspn._abi.TspnError) as e:
        tspn._abi.check(lib.tspn_heads_f32(0, 1, None, 4, None, None, 1, None, 1, None, 17, 1, 4, 4, 1, None))
    assert e.value.code == tspn._abi.TSPN_EUNSUPPORTED and "H=17" in str(e.value)
    assert lib.tspn_conv3_f32(1, 1, -1, 4, 1, 4, None, 0, 1, None) == tspn._abi.TSPN_EINVAL
    assert lib.tspn_pack_conv3_f32(1, 4, 6, 2, 1, None) == tspn._abi.TSPN_EINVAL  # Cin != 2*split
    assert lib.tspn_predicate_head_workspace_bytes(56, 11070, 132) >= 56 * 132 * 4
    d = tspn._abi.FusedDesc()
    d.B, d.N, d.T, d.D, d.A, d.K, d.P = 1, 32, 150, 2048, 4, 132, 992
    need = lib.tspn_forward_fused_workspace_bytes(ctypes.byref(d))
    assert need >= 32 * 8192 * 150 * 4  # the tracklet projections dominate
    assert tspn.ops.fused_workspace_bytes(1, 32, 150, 2048, 4, 132, 992) == need
    d.A = 6  # 3A > 16
    assert lib.tspn_forward_fused_workspace_bytes(ctypes.byref(d)) == 0
    assert lib.tspn_forward_fused_f32(ctypes.byref(d), None) == tspn._abi.TSPN_EUNSUPPORTED


def test_conv_entries_refuse_a_kernel_larger_than_the_padded_map_without_gpu(tspn):
    """(H + 2 pad - KH) / stride + 1 is 1 in C for -stride < H + 2 pad - KH < 0: the four conv entries must refuse such a
    geometry as "empty output" before they look at a pointer (the cases of tests/test_gpu_conv2d_edges.py)."""
    lib = tspn._abi.lib()
    for H, W, KH, KW, stride, pad in [(1, 1, 2, 2, 2, 0), (2, 1, 3, 3, 2, 0), (1, 4, 1, 8, 7, 1)]:
        assert H + 2 * pad < KH or W + 2 * pad < KW
        assert (H + 2 * pad - KH) // stride + 1 <= 0 or (W + 2 * pad - KW) // stride + 1 <= 0
        calls = {
            "tspn_conv2d_nhwc_f32": (None, 2, H, W, 16, None, 32, KH, KW, stride, pad, None, None, 0, None, None),
            "tspn_conv2d_nhwc_frag_f32": (None, 2, H, W, 16, None, 32, KH, KW, stride, pad, None, None, 0, None, None),
            "tspn_conv2d_nhwc_cin4_f32": (None, 2, H, W, None, 32, KH, KW, stride, pad, None, 0, None, None),
            "tspn_conv2d_nhwc_bf16": (None, 2, H, W, 64, None, 32, KH, KW, stride, pad, None, None, 0, None, None),
        }
        for name, args in calls.items():
            assert getattr(lib, name)(*args) == tspn._abi.TSPN_EINVAL, (name, H, W, KH, KW)
            assert (name + ": empty output").encode() in lib.tspn_last_error(), (name, lib.tspn_last_error())
    # a geometry with an output goes on to the pointer check
    assert lib.tspn_conv2d_nhwc_f32(None, 2, 2, 2, 16, None, 32, 2, 2, 2, 0, None, None, 0, None, None) == tspn._abi.TSPN_EINVAL
    assert b"null pointer" in lib.tspn_last_error()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the GPU-less behaviour")
def test_no_cpu_fallback(tspn):
    model = tspn.BaseModel(cases.baseline_cfg())
    model.eval()
    with pytest.raises(RuntimeError, match="no HIP device"):
        model([tspn.PairList(torch.zeros(2, 11070))], None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tspn.ops.predicate_head(torch.zeros(2, 8), torch.zeros(3, 8), None)
    with pytest.raises(RuntimeError):
        tspn.ops.pair_index(4, "cpu")


def test_product_package_never_imports_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "temporal-span-proposal-network-vidvrd_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text, f


def test_hashrng_is_stable(tspn):
    """Known answers: the fixtures depend on these exact streams."""
    u = tspn.hashrng.uniform(0, "x", (4,))
    assert u.dtype == np.float32 and np.all((u >= 0) & (u < 1))
    np.testing.assert_array_equal(u, tspn.hashrng.uniform(0, "x", (4,)))
    assert not np.array_equal(u, tspn.hashrng.uniform(1, "x", (4,)))
    assert not np.array_equal(u, tspn.hashrng.uniform(0, "y", (4,)))
    n = tspn.hashrng.normal(0, "w", (200000,), std=0.01)
    assert abs(float(n.std()) - 0.01) < 1e-4 and abs(float(n.mean())) < 1e-4
    b = tspn.synth.make_video(1, 3, 4, 2)["tracklet_boxes"]
    assert np.all(b == np.round(b)) and np.all(b[..., 2] > b[..., 0]) and np.all(b[..., 3] > b[..., 1])
    assert int(tspn.hashrng.bits(0, "x", 1)[0]) == int(tspn.hashrng.bits(0, "x", 3)[0])


def test_sampler_draws_match_reference_under_the_same_seed(tspn):
    """BalancedPositiveNegativePairSampler (reference relpn/sampler.py:3-66): same masks as the
    reference under torch.manual_seed(1234) (golden g7), quotas respected on ragged inputs."""
    import torch
    import cases
    g = cases.load("g7_misc.npz")
    s = tspn.BalancedPositiveNegativePairSampler(256, 0.25)
    torch.manual_seed(1234)
    labels = [torch.cat([torch.ones(100), torch.zeros(900), -torch.ones(24)]).long(),
              torch.cat([torch.zeros(300), 2 * torch.ones(7)]).long(), torch.zeros(5).long()]
    pos, neg = s(labels)
    for i in range(3):
        assert pos[i].dtype == torch.uint8
        assert (pos[i].numpy() == g[f"sampler_pos_{i}"]).all() and (neg[i].numpy() == g[f"sampler_neg_{i}"]).all()
    assert [int(p.sum()) for p in pos] == [64, 7, 0] and [int(n.sum()) for n in neg] == [192, 249, 5]
    assert int((pos[0][1000:] + neg[0][1000:]).sum()) == 0        # ignored (-1) entries are never drawn
    m = tspn.BaseModel(tspn.load_cfg(None, **{"RELPN.USE_PPN": True}))
    assert isinstance(m.relpn.pair_proposal_network.fg_bg_sampler, tspn.BalancedPositiveNegativePairSampler)


def test_anchor_generator_matches_reference(tspn):
    """AnchorGenerator (reference relpn/anchor_generator.py:31-64) against golden g5; the product's
    span decode enumerates candidates in the same location-major / size-minor order."""
    import torch
    import cases
    g = cases.load("g5_anchors.npz")
    for i, (sizes, stride, tw) in enumerate(cases.G5_SPECS):
        gen = tspn.AnchorGenerator(sizes, stride)
        a = gen(torch.zeros(2, 3, tw))
        assert len(a) == 1 and a[0].dtype == torch.float32
        np.testing.assert_array_equal(a[0].numpy(), g[f"anchors_{i}"])
        assert gen.num_anchors_per_location() == [len(sizes)]
        assert set(gen.state_dict()) == {"cell_anchors_0"}
    gen = tspn.make_anchor_generator(tspn.load_cfg(None))
    assert gen.grid_anchors(60)[0].shape == (len(range(0, 61, 132)) * 4, 2)


def test_weight_caches_are_invalidated(tspn):
    """packed / device copies must not survive load_state_dict, train(), .to() — and
    `invalidate_caches()` exists for in-place `.data` edits that bump no version counter."""
    model = tspn.BaseModel(tspn.load_cfg(None, **{"PREDICT.FEATURE_DIM": 16}))
    cache = model.classifier._cache
    marker = object()
    for action in (lambda: model.load_state_dict(model.state_dict()), lambda: model.train(), lambda: model.eval(),
                   lambda: model.float(), lambda: model.invalidate_caches()):
        cache._store["cls"] = (("stale",), marker)
        action()
        assert "cls" not in cache._store
    p = model.classifier.rel_predictor.weight
    v0 = p._version
    p.data.mul_(2.0)
    assert p._version == v0    # the documented blind spot: .data edits need invalidate_caches()


def test_gt_matrices_truncate_like_zip(tspn):
    """ppn.py:44 zips pairs with labels: the shorter one wins."""
    pl = tspn.PairList(torch.zeros(3, 4))
    pl.add_field("tracklet_pairs", np.array([[0, 1], [1, 2], [2, 0]]))
    pl.add_field("num_tracklets", 3)
    tgt = torch.zeros(5, 6)
    tgt[1, 2] = 1
    tgt[4, 0] = 1            # beyond the pair table: ignored
    gt = tspn.PPN._gt_matrices([pl], [tspn.TargetList(tgt)])[0]
    assert gt.sum() == 1 and gt[1, 2] == 1
    gt = tspn.PPN._gt_matrices([pl], [tspn.TargetList(tgt[:2])])[0]   # fewer labels than pairs
    assert gt.sum() == 1 and gt[1, 2] == 1


def test_on_disk_formats_of_the_reference(tspn, tmp_path):
    """traj_cls JSON (trajectory.py:72-82 / vrdataset.py:162-188) round trip, the reference's file naming, and the
    h5py gate of the -relation.h5 helpers."""
    ds = tspn.dataset
    assert ds.segment_signature("ILSVRC2015_train_00005003", 0, 30) == "ILSVRC2015_train_00005003-0000-0030"
    vsig = ds.segment_signature("v1", 15, 45)
    p = ds.feature_path(str(tmp_path), "traj_cls", "v1", vsig, "json", create=True)
    assert p.endswith(os.path.join("features", "traj_cls", "v1", "v1-0015-0045-traj_cls.json"))
    boxes = np.arange(2 * 30 * 4, dtype=np.float32).reshape(2, 30, 4)
    cls = tspn.hashrng.uniform(3, "cls", (2, 35))
    trajs = ds.tracklets_to_traj_cls(torch.from_numpy(boxes), cls, fstart=15, vsig=vsig)
    assert set(trajs[0]) == {"pstart", "pend", "rois", "score", "category", "classeme", "vsig", "gt_trackid"}
    assert trajs[1]["pend"] - trajs[1]["pstart"] == 30 == len(trajs[1]["rois"]) and trajs[0]["gt_trackid"] == -1
    assert trajs[0]["category"] == int(cls[0].argmax())
    ds.write_traj_cls_json(p, trajs)
    got = ds.read_traj_cls_json(p)                       # logit_only: the [N,35] matrix of vrdataset.py:150-160
    assert got.dtype == np.float32 and np.array_equal(got, cls.astype(np.float32))
    full = ds.read_traj_cls_json(p, logit_only=False)
    assert full[1]["rois"][29] == [float(v) for v in boxes[1, 29]]
    assert ds.read_traj_cls_json(p + ".missing").shape == (0, 0)
    h5 = ds.feature_path(str(tmp_path), "relation", "v1", vsig, "h5", create=True)
    assert ds.read_relation_h5(h5) is None               # absent file: like the reference
    try:
        import h5py  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="h5py"):
            ds.write_relation_h5(h5, [-1, 0], [[0, 1], [1, 0]], np.zeros((2, 8)), np.eye(2))
    else:
        ds.write_relation_h5(h5, [-1, 0], [[0, 1], [1, 0]], np.ones((2, 8)), np.eye(2))
        pairs, feats, iou, tid = ds.read_relation_h5(h5)
        assert pairs.tolist() == [[0, 1], [1, 0]] and feats.dtype == np.float32 and tid.tolist() == [-1, 0]


def test_build_records_kernel_resources_and_no_spills():
    """The build parses hipcc's per-kernel resource remarks into kernel_resources.json next to the library and
    refuses to link when a kernel whose inline asm splits a load from its wait (weights straight into MFMA operand
    registers, s_load'ed head weights) spills or uses scratch: a spill between the two would copy
    registers that are not valid yet."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_tspn_build_t", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "temporal-span-proposal-network-vidvrd_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    res = b.kernel_resources()
    assert len(res) > 40
    guarded = [n for n in res if any(k in n for k in b.NO_SPILL_KERNELS)]
    for want in ("conv3_wino63_kernel", "heads_pairgrid4_kernel", "conv2d_nhwc_bf16_kernel"):
        assert any(want in n for n in guarded), f"{want} not in the resource table"
    assert b.check_no_spill(res) == []
    w63 = next(v for n, v in res.items() if "conv3_wino63_kernel" in n)
    assert w63["vgprs"] + w63["agprs"] <= 512 and w63["scratch_bytes"] == 0
    #  the role-split res4 tail and the one-launch blocks sit at the register limit of two waves per SIMD with
    # hand-counted vmcnt and the store-data fence: guarded, within 256 registers, no scratch
    for want in ("tail_io_bf16_kernel", "bottleneck_block_bf16_kernel"):
        inst = [v for n, v in res.items() if want in n]
        assert inst and any(want in n for n in guarded), f"{want} not guarded"
        assert all(v["vgprs"] + v["agprs"] <= 256 and v["scratch_bytes"] == 0 and v["vgpr_spill"] == 0 for v in inst), (want, inst)
    # the guard itself
    fake = {"conv3_wino63_kernel(float*)": {"vgpr_spill": 3, "sgpr_spill": 0, "scratch_bytes": 12}}
    assert len(b.check_no_spill(fake)) == 1


def test_no_wide_buffer_store_is_followed_by_a_write_of_its_data_registers():
    """ISA lint (tools/lint_store_hazard.py): hipcc does not separate a 128-bit buffer store with an SGPR soffset from a
    following vector write of its data registers, and on MI355X that write can land in the store (round 5: wrong bits in
    0.02 % of the one-launch block's outputs until its epilogue kept the data registers live).  Every kernel of the
    library is compiled to assembly and checked: no such pair within three wait states."""
    import importlib.util
    import os
    import shutil
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not available: nothing to compile to ISA")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("lint_store_hazard", os.path.join(root, "tools", "lint_store_hazard.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    # the linted ISA is the shipped ISA: the tool takes its flags from build.py
    flags = lint.build_flags()
    assert "-O3" in flags and "-ffp-contract=off" in flags and "-fPIC" in flags and "--offload-arch=gfx950" in flags
    import sys
    argv, sys.argv = sys.argv, ["lint_store_hazard.py", "--jobs", "6"]
    try:
        assert lint.main() == 0
    finally:
        sys.argv = argv
    # the checker itself: the form that failed on the hardware is recognised
    bad = """_Zk:
\tbuffer_store_dwordx4 v[32:35], v137, s[4:7], s9 offen
\tv_add_f32_e32 v32, v40, v140
"""
    ok = bad.replace("s9 offen", "0 offen")
    assert len(lint.lint_asm(bad, 3)) == 1 and not lint.lint_asm(ok, 3)
    assert not lint.lint_asm(bad.replace("v_add_f32_e32 v32", "s_nop 2\n\tv_add_f32_e32 v32"), 3)


def test_no_probe_or_ablation_switches_in_the_kernel_sources():
    """README / DESIGN promise that no kernel source carries probe / ablation switches (`tools/strip_probe_blocks.py --check`);
    until round 6 nothing ran that check.  Also: nothing in csrc/ reads the environment."""
    import glob
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "temporal-span-proposal-network-vidvrd_amd", "csrc", "*.hip")) +
                   glob.glob(os.path.join(root, "temporal-span-proposal-network-vidvrd_amd", "csrc", "*.h")))
    assert len(files) >= 20
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "strip_probe_blocks.py"), "--check"] + files,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    for f in files:
        assert "getenv" not in open(f).read(), f"{f} reads the environment"
