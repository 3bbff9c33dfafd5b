"""The span anchor sampler, the parts that need no GPU: the discipline of csrc/spansample/ (kernel variant table, built
sources, no probe blocks, no memset, no environment reads, no conditional blocks, the store-hazard lint, no spills), the entry
point in header / binding / library and its refusals, the numpy restatement (tests/span_sample_reference.py) by hand and
against the quota arithmetic of sampler.py, and the conditions the GPU tests' generated inputs have to meet."""
import ast
import ctypes
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import span_sample_reference as ref
import spansample_kernel_variants
from test_pairlist_bf16_host import _build_module, global_kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd")
CSRC_SS = os.path.join(PKG, "csrc", "spansample")
NEW_SOURCES = sorted(glob.glob(os.path.join(CSRC_SS, "*.hip")) + glob.glob(os.path.join(CSRC_SS, "*.h")))
ENTRIES = {"tspn_span_anchor_sample", "tspn_span_anchor_sample_partials"}


def test_spansample_kernel_table_equals_the_sources_and_names_existing_tests():
    in_source = global_kernels(sorted(glob.glob(os.path.join(CSRC_SS, "*.hip"))))
    assert in_source == {r["kernel"] for r in spansample_kernel_variants.VARIANTS} and len(in_source) == 4
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    seen = set()
    for r in spansample_kernel_variants.VARIANTS:
        key = (r["kernel"], r["inst"])
        assert key not in seen and r["entry"] in ENTRIES and r["when"] and r["align"] and r["tests"], key
        seen.add(key)
        for node in r["tests"]:
            path, _, name = node.partition("::")
            assert name.split("[")[0] in defined.get(path, ()), f"{key}: {node} does not exist"
    # no kernel of the new directory is also defined in an older one: the older tables stay complete
    older = [f for f in glob.glob(os.path.join(PKG, "csrc", "**", "*.hip"), recursive=True) if os.path.dirname(f) != CSRC_SS]
    assert len(older) > 20 and not (global_kernels(sorted(older)) & in_source)
    tool = open(os.path.join(ROOT, "tools", "check_kernel_variants.py")).read()
    assert "spansample_kernel_variants.VARIANTS" in tool and "spanloss_kernel_variants.VARIANTS" in tool
    # the granularities the table and the case list speak of are the kernels'
    text = open(os.path.join(CSRC_SS, "tspn_span_sample.hip")).read()
    consts = {m.group(1): m.group(2).strip() for m in re.finditer(r"constexpr int (\w+) = ([^;]+);", text)}
    assert (consts["THREADS"], consts["PER_THREAD"], consts["CHUNK"]) == ("256", "16", "THREADS * PER_THREAD")
    assert ref.CHUNK == 256 * 16 and ref.OFFSET_THREADS == 256
    assert "dim3(THREADS), 0, s, hist, nchunks, state, offsets" in text        # the offsets kernel's launch width


def test_spansample_sources_are_built_and_carry_no_probe_blocks_memsets_or_environment_reads():
    build = _build_module()
    hips = [f for f in NEW_SOURCES if f.endswith(".hip")]
    assert hips and set(hips) <= set(build.sources())
    assert set(f for f in NEW_SOURCES if f.endswith(".h")) <= set(build._headers())
    for f in NEW_SOURCES:
        text = open(f).read()
        assert "getenv" not in text, f"{f} reads the environment"
        assert "hipMemsetAsync" not in text and "hipMemset" not in text, f"{f}: the kernels write every output themselves"
        assert not re.search(r"^\s*#\s*if", text, flags=re.M), f"{f} has a conditional block (a switch)"
        assert "asm" not in re.sub(r"//[^\n]*", "", text), f"{f}: nothing here needs inline assembly"
        # the only atomics are integer adds on the LDS histogram (arrays named lds_*): none on global memory
        code = re.sub(r"//[^\n]*", "", text)
        uses = re.findall(r"\b\w*[aA]tomic\w*\s*\(\s*([^,)]*)", code)
        assert uses and all(u.startswith("&lds_") for u in uses), uses
        for name in set(re.findall(r"&(lds_\w+)", code)):
            assert re.search(r"__shared__\s+unsigned\s+%s\[" % name, code), name
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "strip_probe_blocks.py"), "--check"] + NEW_SOURCES,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]


def test_store_hazard_lint_passes_on_the_spansample_sources():
    hips = [f for f in NEW_SOURCES if f.endswith(".hip")]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lint_store_hazard.py")] + hips,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-2000:]
    assert all(os.path.basename(f) in res.stdout for f in hips)


def test_new_kernels_do_not_spill():
    res = _build_module().kernel_resources()
    names = {r["kernel"] for r in spansample_kernel_variants.VARIANTS}
    found = {n: r for n, r in res.items() if any(k in n for k in names)}
    assert len(found) == len(names)
    for n, r in found.items():
        assert not (r.get("sgpr_spill", 0) or r.get("vgpr_spill", 0) or r.get("scratch_bytes", 0)), (n, r)


def test_entry_point_is_declared_bound_and_exported_without_scratch_parameters():
    import tspn_mi355x
    abi = tspn_mi355x._abi
    assert ENTRIES <= set(abi.header_symbols()) and ENTRIES <= set(abi.PROTOTYPES)
    handle = ctypes.CDLL(abi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(handle, name), name
    assert "span_anchor_sample" in tspn_mi355x.ops.__all__
    assert abi.lib().tspn_version() == 7                                # the entry only adds symbols
    header = re.sub(r"/\*.*?\*/", " ", open(abi.HEADER_PATH).read(), flags=re.S)
    params = re.search(r"\btspn_span_anchor_sample\s*\(([^;]*?)\)\s*;", header, re.S).group(1)
    assert "workspace" not in params and "tspn_span_anchor_sample_workspace_bytes" not in header
    assert re.sub(r"\s+", " ", params) == ("const int8_t* label, int64_t n, uint64_t stream_key, int key_bits, int64_t batch, "
                                           "int64_t want_pos, uint32_t* partials, int64_t* counts, uint8_t* mask, void* stream")
    cfg = tspn_mi355x.default_cfg().RELPN.DPN.SPAN_LOSS
    assert (cfg.POS_IOU, cfg.NEG_IOU, cfg.SMOOTH_L1_BETA) == (0.7, 0.3, 1.0 / 9.0)
    assert (cfg.BATCH_SIZE_PER_SEGMENT, cfg.POSITIVE_FRACTION, cfg.SAMPLE_SEED) == (0, 0.5, 0)


def test_stream_key_is_the_key_of_hashrng_bits():
    from tspn_mi355x import hashrng
    for seed, tag in ((0, "span_sample/0"), (7, "span_sample/12"), (2 ** 40 + 1, "x")):
        k = hashrng.stream_key(seed, tag)
        assert k == hashrng._key(seed, tag) and 0 <= k < 2 ** 64
        idx = np.arange(5, dtype=np.uint64)
        with np.errstate(over="ignore"):
            words = hashrng._splitmix64(np.uint64(k) + idx * np.uint64(0x9E3779B97F4A7C15))
        assert np.array_equal(words, hashrng.bits(seed, tag, 5))
    assert hashrng.stream_key(0, "span_sample/0") != hashrng.stream_key(0, "span_sample/1")


def test_op_refuses_cpu_tensors_and_wrong_operands():
    import tspn_mi355x
    ops = tspn_mi355x.ops
    lab = torch.zeros((3, 4, 5), dtype=torch.int8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.span_anchor_sample(lab, 256, 0.5, 1)
    with pytest.raises(TypeError):
        ops.span_anchor_sample([0, 1], 256, 0.5, 1)


def test_refusals_are_answered_without_a_device():
    """Every refusal comes from the argument checks, before any device work: the pointers are made-up addresses."""
    import tspn_mi355x
    A_ = tspn_mi355x._abi
    lib = A_.lib()
    p = ctypes.c_void_p
    ok, odd, null = p(0x10000), p(0x10002), p(0)

    def sample(label=ok, n=100, key=1, key_bits=32, batch=256, want_pos=128, partials=ok, counts=ok, mask=ok):
        return (lib.tspn_span_anchor_sample(label, n, key, key_bits, batch, want_pos, partials, counts, mask, null),
                lib.tspn_last_error().decode())

    for kw in ("label", "partials", "counts", "mask"):
        rc, msg = sample(**{kw: null})
        assert rc == A_.TSPN_EINVAL and "null pointer" in msg, kw
    rc, msg = sample(n=-1)
    assert rc == A_.TSPN_EINVAL and "n=-1" in msg
    rc, msg = sample(n=2 ** 31)
    assert rc == A_.TSPN_EUNSUPPORTED and "2^31" in msg
    for kb in (0, -1, 33, 64):
        rc, msg = sample(key_bits=kb)
        assert rc == A_.TSPN_EINVAL and f"key_bits={kb}" in msg
    rc, msg = sample(batch=-1, want_pos=0)
    assert rc == A_.TSPN_EINVAL and "batch=-1" in msg
    for want in (-1, 257):
        rc, msg = sample(want_pos=want)
        assert rc == A_.TSPN_EINVAL and f"want_pos={want}" in msg
    assert sample(counts=odd)[0] == A_.TSPN_EUNSUPPORTED and sample(partials=odd)[0] == A_.TSPN_EUNSUPPORTED
    assert sample(n=0, counts=null)[0] == A_.TSPN_EINVAL                 # n = 0 still writes counts
    # the size function: 0 for the sizes the entry refuses, the state alone for n = 0, 514 words per chunk of 4096 beyond it
    size = lib.tspn_span_anchor_sample_partials
    assert size(-1) == 0 and size(2 ** 31) == 0 and size(2 ** 40) == 0
    assert size(0) == 8 and size(1) == 8 + 514 and size(4096) == 8 + 514 and size(4097) == 8 + 2 * 514
    assert size(2 ** 31 - 1) == 8 + 514 * 2 ** 19


# ------------------------------------------------------------------------------------------- the restatement
def test_restatement_by_hand_on_a_dozen_anchors_with_ties():
    """Twelve anchors, 1-bit keys: four positives (one labelled 2), six negatives, two ignored (-1, -128).  batch 5 with
    want_pos 3: the third positive and the second negative are both decided by the index among equal keys."""
    label = np.array([1, 0, 0, -1, 1, 0, 2, 0, 0, 1, -128, 0], np.int8)
    key = ref.keys_ref(1, "hand", 12, 1)
    assert key.tolist() == [0, 0, 0, 0, 1, 0, 0, 1, 1, 1, 0, 1]
    # positives in (key, index) order: (0, 0), (0, 6), (1, 4), (1, 9) -> 0, 6, 4;  negatives: (0, 1), (0, 2), (0, 5), .. -> 1, 2
    mask, counts, info = ref.sample_ref(label, 1, "hand", 1, batch=5, want_pos=3)
    assert mask.tolist() == [1, 1, 1, 0, 1, 0, 1, 0, 0, 0, 0, 0] and counts.tolist() == [4, 6, 3, 2]
    assert info[0]["equal"].tolist() == [4, 9] and info[0]["taken"] == 1
    assert info[1]["equal"].tolist() == [1, 2, 5] and info[1]["taken"] == 2
    # the same with every key distinct in effect: 64-bit keys cannot be asked of the restatement, 32 are the most
    mask32, counts32, _ = ref.sample_ref(label, 1, "hand", 32, batch=5, want_pos=3)
    k32 = ref.keys_ref(1, "hand", 12, 32).tolist()
    pos = sorted((k32[i], i) for i in (0, 4, 6, 9))[:3]
    neg = sorted((k32[i], i) for i in (1, 2, 5, 7, 8, 11))[:2]
    assert sorted(np.flatnonzero(mask32).tolist()) == sorted(i for _, i in pos + neg) and counts32.tolist() == [4, 6, 3, 2]
    # a shaped label gives a mask of its shape
    assert ref.sample_ref(label.reshape(2, 3, 2), 1, "hand", 1, 5, 3)[0].shape == (2, 3, 2)
    # the radix rounds of a key width, and the round that decides a threshold
    assert [ref.rounds_of(b) for b in (1, 8, 9, 16, 17, 24, 25, 32)] == [1, 1, 2, 2, 3, 3, 4, 4]
    keys = np.array([0x01020304, 0x01020399, 0x01990000, 0x77000000], np.uint64)
    assert [ref.decided_round(keys, int(k), 32) for k in keys] == [3, 3, 1, 0]


def test_restatement_quotas_equal_the_host_samplers():
    """sampler.py's BalancedPositiveNegativePairSampler (the host mirror of the reference's class) on the same class sizes
    selects as many positives and negatives as the restatement's quota rule, with want_pos = int(batch * fraction)."""
    from tspn_mi355x.sampler import BalancedPositiveNegativePairSampler
    combos = [(n_pos, n_neg, batch, f) for n_pos in (0, 1, 3, 128, 200) for n_neg in (0, 2, 128, 500)
              for batch in (0, 1, 7, 256) for f in (0.0, 0.25, 0.5, 1.0)]
    for n_pos, n_neg, batch, f in combos:
        labels = torch.cat([torch.ones(n_pos), torch.zeros(n_neg), -torch.ones(5)]).to(torch.int64)
        pos, neg = BalancedPositiveNegativePairSampler(batch, f)([labels])
        want = ref.quotas_ref(n_pos, n_neg, batch, int(batch * f))
        assert (int(pos[0].sum()), int(neg[0].sum())) == want, (n_pos, n_neg, batch, f)
        assert not bool((pos[0] & neg[0]).any()) and not bool(pos[0][labels < 1].any()) and not bool(neg[0][labels != 0].any())
        mask, counts, _ = ref.sample_ref(labels.numpy().astype(np.int8), 3, "quota", 32, batch, int(batch * f))
        assert counts.tolist() == [n_pos, n_neg, *want] and int(mask.sum()) == sum(want)


def test_generated_inputs_meet_the_conditions_the_gpu_tests_rely_on():
    """With the restatement alone: the sizes, key widths, class mixes and quotas the issue names are all in the case list;
    threshold-equal anchors straddle a chunk boundary with the cut among them; a threshold is decided in every radix round
    of every round count; every quota regime occurs; the full-size case cuts between two anchors of equal 32-bit keys."""
    cases = {c["id"]: c for c in ref.CASES}
    assert len(cases) == len(ref.CASES) and set(ref.ALL_IDS) == set(cases) | {c["id"] for c, _ in ref.special_cases()}
    C = ref.CHUNK
    assert {1, 63, 64, 65, C - 1, C, C + 1, 3 * C + 5} <= {c["n"] for c in ref.CASES}
    assert any(-(-c["n"] // C) > ref.OFFSET_THREADS for c in ref.CASES)
    assert {1, 4, 8, 9, 16, 17, 32} <= {c["key_bits"] for c in ref.CASES}
    assert {(b, f) for b in (0, 1, 256) for f in (0.0, 0.5, 1.0)} <= {(c["batch"], c["fraction"]) for c in ref.CASES}
    decided, regimes, straddles, sizes_with_ties = {}, set(), [], set()
    for cid in ref.ALL_IDS:
        case, label, mask, counts, info = ref.reference(cid)
        assert label.dtype == np.int8 and label.shape == (case["n"],) and mask.dtype == np.uint8
        want = ref.want_pos_of(case)
        assert 0 <= want <= case["batch"]
        assert int(mask[label >= 1].sum()) == counts[2] and int(mask[label == 0].sum()) == counts[3]
        assert not mask[label < 0].any() and counts[2] + counts[3] <= case["batch"]
        regimes.add(ref.regime(counts, case["batch"], want))
        for c, i in info.items():
            decided.setdefault(ref.rounds_of(case["key_bits"]), set()).add(i["decided_round"])
            taken = i["equal"][:i["taken"]]
            assert mask[taken].all() and not mask[i["equal"][i["taken"]:]].any()          # the lower indices of a tie
            if i["taken"] < len(i["equal"]):
                sizes_with_ties.add(case["n"])
                if len(set((taken // C).tolist())) >= 2:
                    straddles.append(cid)
    assert decided == {R: set(range(R)) for R in (1, 2, 3, 4)}, decided
    assert regimes == {"empty batch", "nothing to select", "positives exactly the quota", "both classes short: all taken",
                       "positives short: negatives fill", "both quotas bind"}, regimes
    assert len(straddles) >= 3, straddles
    assert {1025, C + 1, 3 * C + 5, (ref.OFFSET_THREADS + 1) * C + 3} <= sizes_with_ties
    # the class mixes: what each is for
    by_mix = {}
    for c in ref.CASES:
        by_mix.setdefault(c["mix"], []).append(ref.reference(c["id"]))
    assert all(int(r[3][0]) == 0 and int(r[3][1]) > 0 for r in by_mix["no_pos"])
    assert all(int(r[3][1]) == 0 and int(r[3][0]) > 0 for r in by_mix["no_neg"])
    assert all(r[3].tolist() == [0, 0, 0, 0] and not r[2].any() for r in by_mix["only_ignored"])
    assert all(0 < r[3][0] < ref.want_pos_of(r[0]) and r[3][2] + r[3][3] == r[0]["batch"] for r in by_mix["few_pos"])
    assert all(r[3][2] + r[3][3] < r[0]["batch"] and r[3][0] > 0 and r[3][1] > 0 for r in by_mix["both_short"])
    assert all(r[3][0] == ref.want_pos_of(r[0]) == r[3][2] for r in by_mix["exact_pos"])
    assert all(set(np.unique(r[1]).tolist()) >= {-128, -1, 0, 1, 2} for r in by_mix["mixed"] if r[0]["n"] >= 4095)
    # the two constructed cases
    (last, _), (full, full_label) = ref.special_cases()
    info = ref.reference("last-round")[4]
    assert last["key_bits"] == 32 and info[1]["decided_round"] == 3
    _, _, mask, counts, info = ref.reference("full-size-tie")
    assert full["n"] == ref.FULL_N == 595200 and full["key_bits"] == 32 and full_label.shape == (595200,)
    assert len(info[1]["equal"]) == 2 and info[1]["taken"] == 1 and mask[info[1]["equal"]].tolist() == [1, 0]
