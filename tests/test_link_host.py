"""Tracklet linking without a device: the numpy restatement (tests/link_reference.py) on hand-worked cases and on the
scenes the GPU tests run, the kernel variant table of csrc/link/ against the sources, and the return code and whole
tspn_last_error() text of every refusal of the three entries (made-up device addresses: the checks come before any
launch)."""
import ast
import ctypes
import glob
import importlib.util
import os
import re

import numpy as np
import pytest

import link_kernel_variants
import link_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_LK = os.path.join(PKG, "csrc", "link")
ENTRIES = {"tspn_link_detections_f32", "tspn_link_fill_f32", "tspn_link_scratch_bytes"}


def rows(*frames):
    """frames of [(x1, y1, x2, y2)] or [(x1, y1, x2, y2, score, class)] -> the packed detections"""
    full = [[tuple(r) + (0.9, 1) if len(r) == 4 else tuple(r) for r in f] for f in frames]
    return ref.pack(full, max([len(f) for f in full] + [1]))


def link(frames, **kw):
    b, s, c, n = frames
    return ref.link(b, s, c, n, [0, len(n)], **kw)


# ------------------------------------------------------------------------------------------------- hand-worked cases
def test_iou_and_prediction_by_hand():
    iou = ref.iou_f32([0, 0, 4, 4], [[2, 0, 10, 4], [0, 0, 4, 4], [4, 0, 8, 4], [0, 0, 0, 0]])
    assert iou[0] == np.float32(8) / np.float32(40) and iou[1] == 1 and iou[2] == 0 and iou[3] == 0
    assert np.isnan(ref.iou_f32([0, 0, 0, 0], [[0, 0, 0, 0]])[0])                        # 0 / 0: never an edge
    assert np.isnan(ref.iou_f32([np.nan, 0, 4, 4], [[0, 0, 4, 4]])[0])
    last, prev = np.array([30, 0, 40, 10], np.float32), np.array([10, 0, 20, 10], np.float32)
    assert np.array_equal(ref.predict(last, prev, 5, 3, 2, 8), [60, 0, 70, 10])          # 10 px a frame, 3 frames on
    assert np.array_equal(ref.predict(last, prev, 5, 3, 1, 8), last)                     # one hit: no velocity yet
    assert np.array_equal(ref.predict(last, prev, 5, 3, 2, 8, use_velocity=False), last)
    third = ref.predict(np.array([1, 0, 0, 0], np.float32), np.zeros(4, np.float32), 3, 0, 2, 4)
    assert third[0] == np.float32(1) + np.float32(1) / np.float32(3) * np.float32(1)     # the statement order, in fp32


def test_ties_go_to_the_lower_track_then_the_lower_detection():
    # a detection that overlaps two tracks alike (IoU 8 / 40 each)
    res = link(rows([(0, 0, 4, 4), (8, 0, 12, 4)], [(2, 0, 10, 4)]), iou_thresh=0.1, min_hits=1)
    assert list(res["track_of_det"][1][:1]) == [0] and res["n_tracks"][0] == 2 and list(res["hits"][0, :2]) == [2, 1]
    # the same with the tracks born in the other order: still the lower id
    res = link(rows([(8, 0, 12, 4), (0, 0, 4, 4)], [(2, 0, 10, 4)]), iou_thresh=0.1, min_hits=1)
    assert list(res["track_of_det"][1][:1]) == [0] and np.array_equal(res["last"][0, :2], [1, 0])
    # two detections that overlap one track alike: the lower index is taken, the other starts a track
    res = link(rows([(0, 0, 4, 4)], [(1, 0, 5, 4), (1, 0, 5, 4)]), min_hits=1)
    assert list(res["track_of_det"][1]) == [0, 1] and res["n_tracks"][0] == 2
    # the better IoU wins over the lower id and the lower index
    res = link(rows([(0, 0, 4, 4), (3, 0, 7, 4)], [(3, 0, 7, 4), (0, 0, 4, 4)]), iou_thresh=0.1, min_hits=1)
    assert list(res["track_of_det"][1]) == [1, 0]


def test_a_gap_of_max_age_survives_and_one_more_starts_a_new_id():
    box = (10, 10, 50, 50)
    res = link(rows([box], [], [], [box]), min_hits=1, max_age=3)
    assert res["track_of_det"][3, 0] == 0 and res["n_tracks"][0] == 1 and res["hits"][0, 0] == 2 and res["last"][0, 0] == 3
    res = link(rows([box], [], [], [], [box]), min_hits=1, max_age=3)
    assert res["track_of_det"][4, 0] == 1 and res["n_tracks"][0] == 2 and list(res["first"][0, :2]) == [0, 4]
    res = link(rows([box], [box]), min_hits=1, max_age=0)                               # max_age 0: the next frame is too late
    assert res["track_of_det"][1, 0] == 1


def test_a_tentative_track_dies_at_its_first_miss():
    box = (10, 10, 50, 50)
    res = link(rows([box], [], [box]))                                                  # min_hits 3: one hit, one miss
    assert list(res["track_of_det"][:, 0]) == [0, -1, 1]
    res = link(rows([box], [box], [], [box]))                                           # two hits, one miss
    assert list(res["track_of_det"][:, 0]) == [0, 0, -1, 1] and list(res["hits"][0, :2]) == [2, 1]
    res = link(rows([box], [box], [box], [], [box]))                                    # confirmed at the third hit
    assert list(res["track_of_det"][:, 0]) == [0, 0, 0, -1, 0] and res["hits"][0, 0] == 4
    assert res["score"][0, 0] == np.float32(4 * float(np.float32(0.9)) / 4) and res["cls"][0, 0] == 1


def test_births_past_max_live_and_max_tracks_are_dropped():
    five = [(100 * i, 0, 100 * i + 40, 40) for i in range(5)]
    res = link(rows(five, five), min_hits=1, max_live=3)
    assert list(res["track_of_det"][0]) == [0, 1, 2, -1, -1] and list(res["track_of_det"][1]) == [0, 1, 2, -1, -1]
    assert res["n_tracks"][0] == 3 and res["dropped"][0] == 4
    res = link(rows(five, [], five), min_hits=1, max_age=0, max_tracks=7)                # the ids run out, not the slots
    assert list(res["track_of_det"][2]) == [5, 6, -1, -1, -1] and res["n_tracks"][0] == 7 and res["dropped"][0] == 3
    assert res["first"].shape == (1, 7) and list(res["first"][0]) == [0, 0, 0, 0, 0, 2, 2]
    res = link(rows(five), max_live=5, max_tracks=7)
    assert res["dropped"][0] == 0 and list(res["first"][0]) == [0] * 5 + [-1] * 2 and list(res["hits"][0]) == [1] * 5 + [0] * 2


def test_rows_that_are_no_candidates():
    nan, inf = float("nan"), float("inf")
    frame = [(0, 0, 40, 40, 0.9, 1), (100, 0, nan, 40, 0.9, 1), (200, 0, 240, inf, 0.9, 1), (300, 0, 340, 40, nan, 1),
             (400, 0, 440, 40, inf, 1), (500, 0, 540, 40, 0.5, 1), (600, 0, 640, 40, np.nextafter(np.float32(0.5), np.float32(0)), 1)]
    b, s, c, n = ref.pack([frame, frame], 8)
    res = ref.link(b, s, c, n, [0, 2], min_hits=1, min_score=0.5)
    assert list(res["track_of_det"][0]) == [0, -1, -1, -1, -1, 1, -1, -1] and res["dropped"][0] == 0
    n[1] = 5                                                                              # the count cuts row 5 off
    res = ref.link(b, s, c, n, [0, 2], min_hits=1, min_score=0.5)
    assert list(res["track_of_det"][1]) == [0, -1, -1, -1, -1, -1, -1, -1]


def test_both_match_forms_agree_and_the_chain_needs_four_rounds():
    b, s, c, n = ref.chain_frame()
    stats = {}
    res = ref.link(b, s, c, n, [0, 2], min_hits=1, stats=stats)
    assert stats["max_rounds"] >= 4
    # the strongest link is taken first, then every second one down the chain: a round each
    assert list(res["track_of_det"][1]) == [0, 1, 2, 3] and res["n_tracks"][0] == 4
    b6, s6, c6, n6 = ref.chain_frame(links=6)                                            # the chain ends in a track
    res = ref.link(b6, s6, c6, n6, [0, 2], min_hits=1)
    assert list(res["track_of_det"][1][:3]) == [1, 2, 3] and res["n_tracks"][0] == 4     # detection k goes to track k + 1
    rng = np.random.RandomState(5)
    for _ in range(50):                                                                  # tie-heavy integer grids
        iou = (rng.randint(0, 4, (7, 9)) / 4).astype(np.float32)
        edge = iou >= 0.25
        by_rounds, rounds = ref.match_rounds(iou, edge)
        assert by_rounds == ref.match_sorted(iou, edge) and rounds <= 7


# ------------------------------------------------------------------------------------------------------- the scenes
def test_constant_velocity_scene_needs_the_prediction():
    b, s, c, n = ref.constant_velocity_scene()
    res = ref.link(b, s, c, n, [0, 40])
    assert res["n_tracks"][0] == 2 and list(res["hits"][0, :2]) == [37, 40] and res["dropped"][0] == 0
    tb, state = ref.fill(res, b, [0, 40], *ref.confirmed(res))
    assert tb.shape == (2, 40, 4) and list(state[0, 9:13]) == [1, 2, 2, 1] and state[0, 25] == 2 and (state[1] == 1).all()
    assert np.array_equal(tb[0, 10], [400, 100, 480, 180]) and np.array_equal(tb[0, 25], [850, 100, 930, 180])
    without = ref.link(b, s, c, n, [0, 40], use_velocity=False)
    assert without["n_tracks"][0] == 4


@pytest.mark.parametrize("seed", range(8))
def test_generated_scenes_give_one_confirmed_track_per_object(seed):
    b, s, c, n, owner = ref.generated_scene(seed)
    res = ref.link(b, s, c, n, [0, len(n)])
    ids = np.nonzero(res["hits"][0, :res["n_tracks"][0]] >= 3)[0]
    owners = [set(owner[res["track_of_det"] == k].tolist()) for k in ids]
    assert len(ids) == 6 and all(len(o) == 1 for o in owners), (seed, owners)
    assert sorted(next(iter(o)) for o in owners) == list(range(6))                       # no confirmed false positive


def test_fill_and_segment_cut_by_hand():
    box = lambda x: (x, 0, x + 40, 40)                                                   # noqa: E731
    frames = rows([box(0), box(500)], [box(10)], [], [], [box(40), box(500)], [box(50)])
    b, s, c, n = frames
    s[0, 1], s[4, 1] = 0.5, 0.7
    res = ref.link(b, s, c, n, [0, 6], min_hits=1)
    assert res["n_tracks"][0] == 2 and list(res["hits"][0, :2]) == [4, 2]
    sv, st = ref.confirmed(res, 1)
    tb, state = ref.fill(res, b, [0, 6], sv, st)
    assert list(state[0]) == [1, 1, 2, 2, 1, 1] and list(state[1]) == [1, 2, 2, 2, 1, 0]
    assert np.array_equal(tb[0, 2], [20, 0, 60, 40]) and np.array_equal(tb[0, 3], [30, 0, 70, 40])
    assert np.array_equal(tb[1, 2], [500, 0, 540, 40]) and not tb[1, 5].any()
    seg = ref.segment_tracklets(res, tb, sv, st, 0, 0, 5)
    assert list(seg[1]) == [0, 1] and seg[0].shape == (2, 5, 4) and list(seg[2]) == [1, 1]
    assert list(ref.segment_tracklets(res, tb, sv, st, 0, 0, 6)[1]) == [0]               # track 1 ends at frame 4
    assert list(ref.segment_tracklets(res, tb, sv, st, 0, 0, 5, max_tracklets=1)[1]) == [0]   # the better score
    assert ref.segments_of(75) == [(0, 30), (15, 45), (30, 60), (45, 75)] and ref.segments_of(29) == []
    # a selection outside the tables, a track never born and a repeated one
    tb2, st2 = ref.fill(res, b, [0, 6], np.array([0, 3, 0, 0]), np.array([1, 0, 9, 1]))
    assert np.array_equal(tb2[0], tb[1]) and np.array_equal(tb2[3], tb[1]) and not st2[1:3].any()


# ---------------------------------------------------------------------------------------------- sources and entries
def _build_module():
    spec = importlib.util.spec_from_file_location("_tspn_build_lk", os.path.join(PKG, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def global_kernels(paths):
    names = set()
    for path in paths:
        src = re.sub(r"//[^\n]*|/\*.*?\*/", " ", open(path).read(), flags=re.S)
        for m in re.finditer(r"\b__global__\b", src):
            d = re.search(r"\bvoid\s+([A-Za-z_]\w*)\s*\(", src[m.end():])
            assert d, f"{os.path.basename(path)}: cannot parse the kernel at {src[m.start():m.start() + 80]!r}"
            names.add(d.group(1))
    return names


def test_link_kernel_table_equals_the_sources_and_names_existing_tests():
    hips = sorted(glob.glob(os.path.join(CSRC_LK, "*.hip")))
    assert [os.path.basename(f) for f in hips] == ["tspn_link.hip"]
    in_source = global_kernels(hips)
    assert in_source == {r["kernel"] for r in link_kernel_variants.VARIANTS} and len(in_source) == 6
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in link_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["when"] and r["align"] and r["tests"], key
        assert set(r["entry"].split(" / ")) <= ENTRIES, key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"
    older = [f for f in glob.glob(os.path.join(PKG, "csrc", "**", "*.hip"), recursive=True) if os.path.dirname(f) != CSRC_LK]
    assert len(older) > 20 and not (global_kernels(sorted(older)) & in_source)
    assert "link_kernel_variants.VARIANTS" in open(os.path.join(ROOT, "tools", "check_kernel_variants.py")).read()


def test_link_sources_are_built_and_keep_the_discipline():
    build = _build_module()
    hips = sorted(glob.glob(os.path.join(CSRC_LK, "*.hip")))
    assert set(hips) <= set(build.sources())
    assert "-ffp-contract=off" in build.FLAGS and not [f for f in build.FLAGS if "fast" in f]
    text = open(hips[0]).read()
    code = re.sub(r"//[^\n]*", "", text)
    assert "getenv" not in text and "hipMemset" not in text and "hipMalloc" not in text and "Synchronize" not in text
    assert not re.search(r"^\s*#\s*if", text, flags=re.M) and not re.search(r"\basm\b|__asm", code)
    assert "__fdividef" not in code and "__frcp" not in code and "__fmaf" not in code and "fmaf(" not in code
    assert set(re.findall(r"\batomic\w+", code)) == {"atomicMax", "atomicMin"}            # LDS column maxima; the lowest twin row
    res = build.kernel_resources()
    names = {r["kernel"] for r in link_kernel_variants.VARIANTS}
    found = {n: r for n, r in res.items() if any("::" + k + "(" in n for k in names)}
    assert len(found) == len(link_kernel_variants.VARIANTS)
    for n, r in found.items():
        assert not (r.get("vgpr_spill", 0) or r.get("scratch_bytes", 0)), (n, r)
    lds = [r["lds_bytes"] for n, r in found.items() if "link_detections_kernel" in n]
    # boxes 16 K, classes 8 K, column maxima 8 K, scores 4 K, slots 4 K, two int16 per live slot 16 K, 16 wave sums
    # (the block-wide votes add what the compiler keeps for them); under the 64 KB a kernel gets without asking: no L x D matrix
    assert len(lds) == 1 and 1024 * (16 + 8 + 8 + 4 + 4) + 4096 * 4 + 64 <= lds[0] < 64 * 1024


@pytest.fixture(scope="module")
def env():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    return abi, abi.lib()


def test_entries_are_declared_bound_and_exported(env):
    import tspn_mi355x
    abi, lib = env
    assert ENTRIES <= set(abi.header_symbols()) and ENTRIES <= set(abi.PROTOTYPES)
    raw = ctypes.CDLL(abi.LIB_PATH)
    assert all(hasattr(raw, e) for e in ENTRIES) and lib.tspn_version() == abi.ABI_VERSION == 7
    assert {"link_detections", "link_fill"} <= set(tspn_mi355x.ops.__all__)
    for name in ("Tracks", "link_detections", "segment_tracklets", "video_tracklets"):
        assert getattr(tspn_mi355x, name) is getattr(tspn_mi355x.tracklets, name), name
    header = re.sub(r"/\*.*?\*/", " ", open(abi.HEADER_PATH).read(), flags=re.S)
    for entry in ENTRIES:
        params = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % entry, header, re.S).group(1)
        assert len(params.split(",")) == len(abi.PROTOTYPES[entry][1]), entry


vp = ctypes.c_void_p
OK, NULL, ODD4 = vp(0x10000), vp(0), vp(0x10004)


def offs(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_link_detections_refusals(env):
    A_, lib = env
    w = "tspn_link_detections_f32: "
    ins = ("boxes", "scores", "classes", "count")
    outs = ("tod", "n_tracks", "dropped", "first", "last", "hits", "cls", "score")

    def run(off=(0, 40, 40, 100), V=None, F=100, D=100, thr=0.3, max_age=30, min_hits=3, min_score=0.0, max_live=1024,
            max_tracks=16384, scratch=OK, nbytes=1 << 30, **ptr):
        arr = None if off is None else offs(*off)
        V = (len(off) - 1 if off is not None else 3) if V is None else V
        rc = lib.tspn_link_detections_f32(*[ptr.get(n, OK) for n in ins], arr, V, F, D, thr, max_age, min_hits, min_score, 1,
                                          max_live, max_tracks, *[ptr.get(n, OK) for n in outs], scratch, nbytes, None)
        return rc, lib.tspn_last_error().decode()

    sizes = w + "bad sizes V=%d F=%d D=%d max_live=%d max_tracks=%d"
    assert run(V=-1) == (A_.TSPN_EINVAL, sizes % (-1, 100, 100, 1024, 16384))
    assert run(F=-1) == (A_.TSPN_EINVAL, sizes % (3, -1, 100, 1024, 16384))
    assert run(D=0) == (A_.TSPN_EINVAL, sizes % (3, 100, 0, 1024, 16384))
    assert run(max_live=0)[0] == run(max_tracks=0)[0] == A_.TSPN_EINVAL
    assert run(D=1025) == (A_.TSPN_EUNSUPPORTED, w + "D=1025 > 1024")
    assert run(D=1024, scratch=NULL)[0] == A_.TSPN_EWORKSPACE                             # 1024 itself is served
    assert run(max_live=4097) == (A_.TSPN_EUNSUPPORTED, w + "max_live=4097 > 4096")
    assert run(max_live=4096, scratch=NULL)[0] == A_.TSPN_EWORKSPACE
    assert run(max_tracks=1 << 24) == run(F=1 << 21, off=(0, 1 << 21)) == (A_.TSPN_EUNSUPPORTED, w + "dimension too large")
    rule = w + "iou_thresh must lie in (0, 1]"
    for thr in (0.0, -0.5, 1.5, float("nan"), float("inf")):
        assert run(thr=thr) == (A_.TSPN_EINVAL, rule), thr
    assert run(thr=1.0, scratch=NULL)[0] == A_.TSPN_EWORKSPACE                            # 1 itself is served
    rule = w + "needs max_age >= 0, min_hits >= 1 and min_score a number"
    assert run(max_age=-1) == run(min_hits=0) == run(min_score=float("nan")) == (A_.TSPN_EINVAL, rule)
    # the video offsets, read on the host
    assert run(off=None) == (A_.TSPN_EINVAL, w + "null pointer")
    bad = w + "video_off must ascend from 0 to F=100"
    assert run(off=(0, 60, 40, 100)) == (A_.TSPN_EINVAL, bad)                             # decreasing
    assert run(off=(1, 40, 40, 100)) == run(off=(0, 40, 40, 99)) == run(off=(0, 40, 40, 101)) == (A_.TSPN_EINVAL, bad)
    for n in ins + outs:
        assert run(**{n: NULL}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    align = w + "boxes and scratch must be 16-byte aligned"
    assert run(boxes=ODD4) == run(scratch=ODD4) == (A_.TSPN_EUNSUPPORTED, align)
    # the scratch last: offsets 4 x 8 -> 256, five 16-byte records per slot of 3 x 1024
    need = lib.tspn_link_scratch_bytes(3, 1024, 16384, 0, 0, 0)
    assert need == 256 + 5 * 3 * 1024 * 16
    assert run(nbytes=need - 1) == (A_.TSPN_EWORKSPACE, w + f"scratch {need - 1} < {need} bytes")
    assert run(nbytes=0) == run(scratch=NULL) == (A_.TSPN_EWORKSPACE, w + f"scratch 0 < {need} bytes")
    # the order of the checks decides which error a doubly wrong call gets
    assert "bad sizes" in run(V=-1, D=2000)[1] and "D=2000" in run(D=2000, max_live=5000)[1]
    assert "iou_thresh" in run(thr=0.0, off=(0, 60, 40, 100))[1] and "video_off" in run(off=(0, 60, 40, 100), boxes=NULL)[1]
    assert "null pointer" in run(boxes=NULL, scratch=NULL)[1]
    # no video: nothing to do, no pointer needed; no frame: the inputs are not read
    nothing = {n: NULL for n in ins + outs}
    assert run(off=(0,), F=0, scratch=NULL, nbytes=0, **nothing)[0] == A_.TSPN_OK
    assert run(off=(0, 0), F=0, scratch=NULL, **{n: NULL for n in ins + ("tod",)})[0] == A_.TSPN_EWORKSPACE
    q = lib.tspn_link_scratch_bytes
    assert q(0, 1024, 16384, 0, 0, 0) == 0 and q(3, 4097, 16384, 0, 0, 0) == 0 and q(3, 0, 16384, 0, 0, 0) == 0
    assert q(3, 1024, 1 << 24, 0, 0, 0) == 0 and q(-1, 1024, 16384, 0, 0, 0) == 0


def test_link_fill_refusals(env):
    A_, lib = env
    w = "tspn_link_fill_f32: "
    names = ("boxes", "tod", "first", "last", "sel_video", "sel_track", "out", "state")

    def run(off=(0, 40, 40, 100), V=None, F=100, D=100, max_tracks=16384, R=5, scratch=OK, nbytes=1 << 30, **ptr):
        arr = None if off is None else offs(*off)
        V = (len(off) - 1 if off is not None else 3) if V is None else V
        g = lambda n: ptr.get(n, OK)                                                     # noqa: E731
        rc = lib.tspn_link_fill_f32(g("boxes"), g("tod"), arr, V, F, D, g("first"), g("last"), max_tracks, g("sel_video"),
                                    g("sel_track"), R, g("out"), g("state"), scratch, nbytes, None)
        return rc, lib.tspn_last_error().decode()

    assert run(V=-1) == (A_.TSPN_EINVAL, w + "bad sizes V=-1 F=100 D=100 max_live=1 max_tracks=16384")
    assert run(D=0)[0] == run(max_tracks=0)[0] == A_.TSPN_EINVAL
    assert run(R=-1) == (A_.TSPN_EINVAL, w + "bad sizes R=-1")
    assert run(D=1025) == (A_.TSPN_EUNSUPPORTED, w + "D=1025 > 1024")
    assert run(off=None) == (A_.TSPN_EINVAL, w + "null pointer")
    assert run(off=(0, 60, 40, 100)) == (A_.TSPN_EINVAL, w + "video_off must ascend from 0 to F=100")
    assert run(R=1 << 26) == (A_.TSPN_EUNSUPPORTED, w + "dimension too large")           # R x Fmax past 2^31
    for n in names:
        assert run(**{n: NULL}) == (A_.TSPN_EINVAL, w + "null pointer"), n
    align = w + "boxes, out_boxes and scratch must be 16-byte aligned"
    assert run(boxes=ODD4) == run(out=ODD4) == run(scratch=ODD4) == (A_.TSPN_EUNSUPPORTED, align)
    # offsets 4 x 8 -> 256, rowof 3 x 16384 x 4, hit 5 x 60 x 4 -> 1280
    need = lib.tspn_link_scratch_bytes(3, 0, 16384, 5, 60, 1)
    assert need == 256 + 3 * 16384 * 4 + 1280
    assert run(nbytes=need - 1) == (A_.TSPN_EWORKSPACE, w + f"scratch {need - 1} < {need} bytes")
    assert run(scratch=NULL) == (A_.TSPN_EWORKSPACE, w + f"scratch 0 < {need} bytes")
    nothing = {n: NULL for n in names}
    assert run(R=0, scratch=NULL, **nothing)[0] == run(off=(0, 0), F=0, scratch=NULL, **nothing)[0] == A_.TSPN_OK
    q = lib.tspn_link_scratch_bytes
    assert q(3, 0, 16384, 0, 60, 1) == 0 and q(0, 0, 16384, 5, 60, 1) == 0 and q(3, 0, 16384, 1 << 26, 60, 1) == 0
    assert q(3, 0, 16384, 5, 0, 1) == 256 + 3 * 16384 * 4


def test_wrappers_refuse_before_the_library(env):
    import torch

    import tspn_mi355x
    ops = tspn_mi355x.ops
    det = (torch.zeros(2, 3, 4), torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.link_detections(*det)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tspn_mi355x.link_detections(det)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.link_fill(det[0], torch.zeros(2, 3, dtype=torch.int32), None, None, None, None)
