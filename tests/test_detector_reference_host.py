"""The detector's numpy restatement (tests/detector_reference.py) against hand-worked cases, the kernel variant table of
csrc/detect/ against the sources, and FasterRCNNC4's state-dict keys against detectron2's names.  No device."""
import ast
import glob
import importlib.util
import math
import os
import re

import numpy as np

import detect_kernel_variants
import detector_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_DT = os.path.join(PKG, "csrc", "detect")
ENTRIES = {"tspn_rpn_decode_f32", "tspn_box_head_decode_f32", "tspn_box_nms_f32", "tspn_detections_topk_f32"}


def _build_module():
    spec = importlib.util.spec_from_file_location("_tspn_build_dt", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------- anchors
def test_default_cell_anchors_equal_the_closed_form():
    import tspn_mi355x
    cell = ref.cell_anchors()
    assert cell.shape == (15, 4) and cell.dtype == np.float32
    f = np.float32
    for i, size in enumerate((32, 64, 128, 256, 512)):
        # ratio 0.5: w = size sqrt 2, h = size / sqrt 2;  ratio 1: a square;  ratio 2: the transpose of ratio 0.5
        long_, short = f(size * math.sqrt(2.0) / 2.0), f(size / math.sqrt(2.0) / 2.0)
        assert np.array_equal(cell[3 * i], np.array([-long_, -short, long_, short], f))
        assert np.array_equal(cell[3 * i + 1], np.array([-size / 2, -size / 2, size / 2, size / 2], f))
        assert np.array_equal(cell[3 * i + 2], np.array([-short, -long_, short, long_], f))
    assert np.array_equal(tspn_mi355x.generate_cell_anchors_2d().numpy(), cell)
    assert np.array_equal(tspn_mi355x.generate_cell_anchors_2d((8,), (1.0, 4.0)).numpy(), ref.cell_anchors((8,), (1.0, 4.0)))
    # flat index (h W + w) A + a = cell anchor a + (w, h, w, h) * stride
    g = ref.grid_anchors(cell, 3, 5, 16)
    assert g.shape == (3 * 5 * 15, 4)
    h, w, a = 2, 3, 7
    assert np.array_equal(g[(h * 5 + w) * 15 + a], cell[a] + np.array([48, 32, 48, 32], f))


# -------------------------------------------------------------------------------------------------------- decode
def test_apply_deltas_by_hand():
    box = np.array([[10, 20, 30, 60]], np.float32)                          # w 20, h 40, centre (20, 40)
    out, mx, my = ref.apply_deltas(box, np.zeros((1, 4), np.float32), (1, 1, 1, 1))
    assert np.array_equal(out, box) and mx[0] == 40 and my[0] == 80
    out, _, _ = ref.apply_deltas(box, np.array([[5, -10, 0, 0]], np.float32), (10, 10, 5, 5))      # dx 0.5, dy -1
    assert np.array_equal(out, np.array([[20, -20, 40, 20]], np.float32))
    big, _, _ = ref.apply_deltas(box, np.array([[0, 0, 100, np.inf]], np.float32), (1, 1, 1, 1), np.float64)
    assert np.allclose(big[0, 2] - big[0, 0], 62.5 * 20, rtol=1e-7) and np.allclose(big[0, 3] - big[0, 1], 62.5 * 40, rtol=1e-7)
    nan, _, _ = ref.apply_deltas(box, np.array([[0, 0, np.nan, 0]], np.float32), (1, 1, 1, 1))
    assert np.isnan(nan[0, 0]) and np.isnan(nan[0, 2]) and np.isfinite(nan[0, 1])
    c = ref.clip(np.array([[-5, -1, 200, 50], [np.nan, 3, 4, 500]], np.float32), np.float32(100), np.float32(120))
    assert np.array_equal(c[0], [0, 0, 120, 50]) and np.isnan(c[1, 0]) and c[1, 3] == 100


def test_box_head_restatement_by_hand():
    z = np.array([[0, 0, 0, 0], [np.log(2), 0, 0, 0], [0, np.nan, 0, 0], [1, 2, 3, 4]], np.float32)   # K = 3, background last
    props = np.tile(np.array([[[10, 10, 30, 50]]], np.float32), (1, 4, 1))
    deltas = np.zeros((4, 12), np.float32)
    sizes = np.array([[40, 100]], np.float32)
    s, b, v, row_ok, _, raw = ref.box_head_decode(z, deltas, props, np.array([3]), sizes, 0.25, dtype=np.float64)
    assert s.shape == (1, 3, 4) and b.shape == (1, 3, 4, 4)                            # class-major
    assert list(row_ok[0]) == [True, True, False, False]                              # a NaN row, a row past the count
    assert np.allclose(raw[0, :, 1], [0.4, 0.2, 0.2]) and list(v[0, :, 1]) == [1, 0, 0]   # above the threshold: class 0 only
    assert np.allclose(s[0, :, 1], [0.4, 0, 0])                                        # an absent row's score is 0
    assert not v[0, :, 0].any() and not s[0, :, 0].any()                               # 0.25 is not above 0.25
    assert np.array_equal(b[0, 0, 0], [10, 10, 30, 40]) and not b[0, :, 2:].any()      # clipped; dropped rows are zero


# ----------------------------------------------------------------------------------------------------------- NMS
def test_iou_exactly_at_the_threshold():
    a, b = np.array([0, 0, 2, 1], np.float32), np.array([[0, 0, 1, 1]], np.float32)
    assert not ref.suppresses(a, b, 0.5)[0]                                            # IoU = 0.5, strict comparison
    assert ref.suppresses(a, b, np.nextafter(np.float32(0.5), np.float32(0)))[0]
    assert not ref.suppresses(np.array([0, 0, 0, 0], np.float32), np.zeros((1, 4), np.float32), 0.0)[0]     # 0 / 0
    boxes = np.array([[0, 0, 2, 1], [0, 0, 1, 1]], np.float32)
    s = np.array([2, 1], np.float32)
    assert list(ref.box_nms(boxes, s, None, [0, 2], 2, 0.5, 2, 0.0)[0][0]) == [0, 1]
    assert list(ref.box_nms(boxes, s, None, [0, 2], 2, 0.49, 2, 0.0)[0][0]) == [0, -1]


def test_selection_order():
    s = np.array([1.0, np.nan, 3.0, 3.0, -np.inf, np.inf, -0.0, 0.0, np.nan], np.float32)
    assert list(ref.select_order(s, 9)) == [1, 8, 5, 2, 3, 0, 6, 7, 4]     # NaN first, ties to the lower index, -0 == +0
    assert list(ref.select_order(s, 3)) == [1, 8, 5]
    key = ref.order_key(s)
    assert key[1] == key[8] == 0xffffffff and key[6] == key[7] and key.min() > 0
    same = np.tile(np.array([[0, 0, 4, 4]], np.float32), (5, 1))
    idx, cnt, keep = ref.box_nms(same, np.ones(5, np.float32), None, [0, 5], 5, 0.5, 5, 0.0)
    assert list(idx[0]) == [0, -1, -1, -1, -1] and cnt[0] == 1 and list(keep) == [1, 0, 0, 0, 0]
    idx, cnt, _ = ref.box_nms(None, s, None, [0, 4, 9], 3, 0.0, 3, 0.0)            # the selection alone, two groups
    assert [list(r) for r in idx] == [[1, 2, 3], [8, 5, 6]] and list(cnt) == [3, 3]


def test_suppression_chains_groups_and_min_size():
    chain = np.array([[0, 0, 4, 4], [1, 0, 5, 4], [2, 0, 6, 4]], np.float32)       # IoU(A,B) = IoU(B,C) = 0.6, IoU(A,C) = 1/3
    s = np.array([3, 2, 1], np.float32)
    assert list(ref.box_nms(chain, s, None, [0, 3], 3, 0.5, 3, 0.0)[0][0]) == [0, 2, -1]     # A kills B, so B cannot kill C
    assert list(ref.box_nms(chain, s[::-1].copy(), None, [0, 3], 3, 0.5, 3, 0.0)[0][0]) == [2, 0, -1]
    # the same boxes in two groups never interact
    idx, cnt, _ = ref.box_nms(chain, s, None, [0, 1, 3], 3, 0.5, 3, 0.0)
    assert [list(r) for r in idx] == [[0, -1, -1], [1, -1, -1]] and list(cnt) == [1, 1]
    idx, cnt, _ = ref.box_nms(chain, s, None, [0, 2, 2, 3], 3, 0.5, 2, 0.0)         # an empty group in the middle
    assert [list(r) for r in idx] == [[0, -1], [-1, -1], [2, -1]] and list(cnt) == [1, 0, 1]
    # post_topk stops the scan; pre_topk cuts before anything else
    apart = np.array([[10 * i, 0, 10 * i + 4, 4] for i in range(6)], np.float32)
    assert list(ref.box_nms(apart, np.arange(6, dtype=np.float32), None, [0, 6], 6, 0.5, 2, 0.0)[0][0]) == [5, 4]
    assert list(ref.box_nms(apart, np.arange(6, dtype=np.float32), None, [0, 6], 3, 0.5, 6, 0.0)[0][0]) == [5, 4, 3, -1, -1, -1]
    # min_size: width <= min_size or height <= min_size drops; a negative min_size switches the filter off
    sized = np.array([[0, 0, 2, 9], [20, 0, 23, 3], [40, 0, 40, 5], [60, 0, 64, 4]], np.float32)
    s4 = np.array([4, 3, 2, 1], np.float32)
    assert list(ref.box_nms(sized, s4, None, [0, 4], 4, 0.5, 4, 0.0)[0][0]) == [0, 1, 3, -1]
    assert list(ref.box_nms(sized, s4, None, [0, 4], 4, 0.5, 4, 2.0)[0][0]) == [1, 3, -1, -1]
    assert list(ref.box_nms(sized, s4, None, [0, 4], 4, 0.5, 4, 3.0)[0][0]) == [3, -1, -1, -1]
    assert list(ref.box_nms(sized, s4, None, [0, 4], 4, 0.5, 4, -1.0)[0][0]) == [0, 1, 2, 3]


def test_non_finite_rows_are_dropped_after_the_topk():
    """detectron2's find_top_rpn_proposals takes the top-k first and drops non-finite rows then: a dropped row is not
    replaced from below the cut."""
    H, W, A = 1, 4, 1
    cell = np.array([[-4, -4, 4, 4]], np.float32)
    logits = np.array([4, 3, 2, 1], np.float32).reshape(1, H, W, A)
    deltas = np.zeros((1, H, W, 4), np.float32)
    deltas[0, 0, 1, 2] = np.nan                                                     # the second best candidate
    sizes = np.array([[100, 100]], np.float32)
    cand = ref.rpn_proposals_select(logits, 3)
    assert list(cand[0]) == [0, 1, 2]
    boxes, lg, valid, _ = ref.rpn_decode(cand, logits, deltas, cell, 16, sizes)
    assert list(valid[0]) == [1, 0, 1] and not boxes[0, 1].any()
    ob, ol, cnt = ref.rpn_proposals_finish(boxes, lg, valid, 3, 0.7, 0.0)
    assert cnt[0] == 2 and list(ol[0]) == [4, 2, 0]                                 # candidate 3 (logit 1) does not move up
    assert np.array_equal(ob[0, 0], [0, 0, 4, 4]) and np.array_equal(ob[0, 1], [28, 0, 36, 4]) and not ob[0, 2].any()
    inf = logits.copy()
    inf[0, 0, 3, 0] = np.inf                                                        # an infinite logit: selected first, then dropped
    cand = ref.rpn_proposals_select(inf, 2)
    assert list(cand[0]) == [3, 0] and list(ref.rpn_decode(cand, inf, deltas, cell, 16, sizes)[2][0]) == [0, 1]


def test_detections_by_hand():
    scores = np.array([[[0.9, 0.5, 0.0], [0.5, 0.8, 0.5]]], np.float32)             # [B=1, K=2, R=3]
    valid = (scores > 0).astype(np.uint8)
    far = np.array([[0, 0, 4, 4], [10, 0, 14, 4], [20, 0, 24, 4]], np.float32)
    boxes = np.stack([far, far + 100])[None]
    ob, os_, oc, cnt = ref.detections_finish(scores, boxes, valid, 0.5, 4)
    assert cnt[0] == 4 and list(os_[0]) == [0.9, 0.8, 0.5, 0.5] and list(oc[0]) == [0, 1, 1, 0]
    # the three 0.5s: (r 0, c 1) = 1, (r 1, c 0) = 2, (r 2, c 1) = 5 -> the two lowest r K + c
    assert np.array_equal(ob[0, 2], far[0] + 100) and np.array_equal(ob[0, 3], far[1])
    ob, os_, oc, cnt = ref.detections_finish(scores, np.tile(far[0], (1, 2, 3, 1)), valid, 0.5, 4)
    assert cnt[0] == 2 and list(os_[0]) == [0.9, 0.8, 0, 0] and list(oc[0]) == [0, 1, 0, 0]   # NMS per class only


# ------------------------------------------------------------------------------------------------------- sources
def global_kernels(paths):
    """Names of every `__global__` function defined in the given sources (the parse of test_kernel_variant_table.py)."""
    names = set()
    for path in paths:
        src = re.sub(r"//[^\n]*|/\*.*?\*/", " ", open(path).read(), flags=re.S)
        for m in re.finditer(r"\b__global__\b", src):
            d = re.search(r"\bvoid\s+([A-Za-z_]\w*)\s*\(", src[m.end():])
            assert d, f"{os.path.basename(path)}: cannot parse the kernel at {src[m.start():m.start() + 80]!r}"
            names.add(d.group(1))
    return names


def test_detect_kernel_table_equals_the_sources_and_names_existing_tests():
    hips = sorted(glob.glob(os.path.join(CSRC_DT, "*.hip")))
    assert [os.path.basename(f) for f in hips] == ["tspn_detect.hip"]
    in_source = global_kernels(hips)
    assert in_source == {r["kernel"] for r in detect_kernel_variants.VARIANTS} and len(in_source) == 7
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in detect_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] in ENTRIES and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"
    # the one template among them: both instantiations have a row
    assert {r["inst"] for r in detect_kernel_variants.VARIANTS if r["kernel"] == "box_nms_select_kernel"} == {"false", "true"}
    older = [f for f in glob.glob(os.path.join(PKG, "csrc", "**", "*.hip"), recursive=True) if os.path.dirname(f) != CSRC_DT]
    assert len(older) > 20 and not (global_kernels(sorted(older)) & in_source)
    assert "detect_kernel_variants.VARIANTS" in open(os.path.join(ROOT, "tools", "check_kernel_variants.py")).read()


def test_detect_sources_are_built_and_keep_the_discipline():
    build = _build_module()
    hips = sorted(glob.glob(os.path.join(CSRC_DT, "*.hip")))
    assert set(hips) <= set(build.sources())
    assert "-ffp-contract=off" in build.FLAGS and not [f for f in build.FLAGS if "fast" in f]
    text = open(hips[0]).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "getenv" not in text and "hipMemset" not in text and "hipMalloc" not in text and "Synchronize" not in text
    assert not re.search(r"^\s*#\s*if", text, flags=re.M) and not re.search(r"\basm\b|__asm", code)
    assert '#include "tspn_topk_select.h"' in text and "select_topk_sorted" in code       # selection has one home
    assert not re.search(r"bitonic|hist\[", code), "a second copy of the selection"
    assert "__expf" not in code and "__fdividef" not in code and "__frcp" not in code     # expf and a true division
    assert set(re.findall(r"\batomic\w+", code)) == {"atomicAdd"}                         # an integer count in LDS
    res = build.kernel_resources()
    names = {r["kernel"] for r in detect_kernel_variants.VARIANTS}
    found = {n: r for n, r in res.items() if any(k + "(" in n or k + "<" in n for k in names)}
    assert len(found) == len(detect_kernel_variants.VARIANTS)
    for n, r in found.items():
        assert not (r.get("sgpr_spill", 0) or r.get("vgpr_spill", 0) or r.get("scratch_bytes", 0)), (n, r)
    big = [r["lds_bytes"] for n, r in found.items() if "box_nms_select_kernel" in n]
    assert big == [256 * 4 + 12 + 2 * 8192 * 4] * 2                                      # the 8192-pair selection: 65 KB of LDS


def test_entries_are_declared_bound_and_exported():
    import ctypes

    import tspn_mi355x
    abi = tspn_mi355x._abi
    every = ENTRIES | {"tspn_box_nms_scratch_bytes"}
    assert every <= set(abi.header_symbols()) and every <= set(abi.PROTOTYPES)
    raw = ctypes.CDLL(abi.LIB_PATH)
    assert all(hasattr(raw, e) for e in every) and abi.lib().tspn_version() == abi.ABI_VERSION == 7
    assert {"rpn_decode", "box_head_decode", "box_nms", "rpn_proposals", "box_detections"} <= set(tspn_mi355x.ops.__all__)
    assert tspn_mi355x.FasterRCNNC4 is tspn_mi355x.detector.FasterRCNNC4
    header = re.sub(r"/\*.*?\*/", " ", open(abi.HEADER_PATH).read(), flags=re.S)
    for entry in every:
        params = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % entry, header, re.S).group(1)
        assert len(params.split(",")) == len(abi.PROTOTYPES[entry][1]), entry


# ----------------------------------------------------------------------------------------------------- the module
def test_state_dict_keys_are_detectron2s():
    """The keys of detectron2 v0.6's faster_rcnn_R_50_C4 state dict, written out: GeneralizedRCNN's pixel_mean / pixel_std
    and the anchor generator's cell anchors are non-persistent buffers there and take no part."""
    import torch

    import tspn_mi355x

    def conv_bn(prefix):
        return [prefix + ".weight"] + [f"{prefix}.norm.{n}" for n in ("weight", "bias", "running_mean", "running_var")]

    def stage(prefix, nblocks):
        keys = []
        for b in range(nblocks):
            for c in (["shortcut"] if b == 0 else []) + ["conv1", "conv2", "conv3"]:
                keys += conv_bn(f"{prefix}.{b}.{c}")
        return keys

    want = conv_bn("backbone.stem.conv1")
    for name, n in (("res2", 3), ("res3", 4), ("res4", 6)):
        want += stage("backbone." + name, n)
    for m in ("conv", "objectness_logits", "anchor_deltas"):
        want += [f"proposal_generator.rpn_head.{m}.weight", f"proposal_generator.rpn_head.{m}.bias"]
    want += stage("roi_heads.res5", 3)
    for m in ("cls_score", "bbox_pred"):
        want += [f"roi_heads.box_predictor.{m}.weight", f"roi_heads.box_predictor.{m}.bias"]
    model = tspn_mi355x.FasterRCNNC4(num_classes=35, depth=50)
    sd = model.state_dict()
    assert list(sd) == want
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    assert shapes["proposal_generator.rpn_head.conv.weight"] == (1024, 1024, 3, 3)
    assert shapes["proposal_generator.rpn_head.objectness_logits.weight"] == (15, 1024, 1, 1)
    assert shapes["proposal_generator.rpn_head.anchor_deltas.weight"] == (60, 1024, 1, 1)
    assert shapes["roi_heads.box_predictor.cls_score.weight"] == (36, 2048)
    assert shapes["roi_heads.box_predictor.bbox_pred.weight"] == (140, 2048)
    assert shapes["roi_heads.res5.0.shortcut.weight"] == (2048, 1024, 1, 1)
    # a detectron2-named state dict round-trips strictly; a missing or a foreign key is an error
    other = tspn_mi355x.FasterRCNNC4(num_classes=35, depth=50)
    given = {k: torch.full_like(v, 0.5) for k, v in sd.items()}
    assert not any(other.load_state_dict(given, strict=True))
    assert all(bool((v == 0.5).all()) for v in other.state_dict().values())
    import pytest
    with pytest.raises(RuntimeError):
        other.load_state_dict({k: v for k, v in given.items() if k != want[-1]}, strict=True)
    with pytest.raises(RuntimeError):
        other.load_state_dict(dict(given, pixel_mean=torch.zeros(3, 1, 1)), strict=True)
    assert tuple(model.pixel_mean.shape) == (3, 1, 1) and len(tspn_mi355x.FasterRCNNC4(depth=101).backbone.res4) == 23
