"""The workspace contract table (tests/workspace_contracts.py) stays equal to include/tspn_mi355x.h and points at tests
that exist, and -- without a device -- every size helper agrees with the `need` its entry computes and returns 0 for
the shapes the entry refuses.

Helper against entry: an entry answers a workspace of 0 bytes with TSPN_EWORKSPACE before any device work and says in
its message how many bytes it wanted ("workspace 0 < N bytes"); N must be what the helper returns for the same shape.
The operands are one 256-byte aligned host address that no entry reads before that answer."""
import ast
import ctypes
import glob
import os
import re

import pytest

import workspace_contracts as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tspn_mi355x.h")


def header_text():
    return re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)


def header_functions():
    """{name: parameter text} of every function declared in the header."""
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(tspn_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", header_text(), re.S)}


def header_structs():
    """{struct name: body} of the descriptor structs."""
    return {m.group(1): m.group(2) for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\w+\s*;", header_text(), re.S)}


def test_header_parser_sees_the_header():
    fns = header_functions()
    assert len(fns) > 80 and "void* workspace" in fns["tspn_decode_topk_f32"]
    assert set(header_structs()) == {"tspn_fused_desc", "tspn_fused_bf16_desc"}


def test_every_workspace_taking_entry_has_exactly_one_row():
    fns, structs = header_functions(), header_structs()
    with_ws = {s for s, body in structs.items() if re.search(r"\bvoid\s*\*\s*workspace\s*;", body)}
    assert with_ws == {"tspn_fused_desc", "tspn_fused_bf16_desc"}
    by_param = {n for n, params in fns.items() if re.search(r"\bvoid\s*\*\s*workspace\b", params)}
    by_desc = {n: s for n, params in fns.items() for s in with_ws
               if re.search(r"\bconst\s+%s\s*\*" % s, params) and not n.endswith("_workspace_bytes")}
    assert len(by_param) >= 12 and len(by_desc) == 3
    rows = [r["entry"] for r in wc.ROWS]
    assert len(rows) == len(set(rows)), "an entry with two rows"
    assert set(rows) == by_param | set(by_desc), (sorted(set(rows) - by_param - set(by_desc)),
                                                  sorted((by_param | set(by_desc)) - set(rows)))
    for r in wc.ROWS:
        assert r["desc"] == by_desc.get(r["entry"]), r["entry"]
        assert r["holds"] and r["zeroed"] and r["wrapper"] and r["tests"], r["entry"]
    assert {r["desc"] for r in wc.ROWS if r["desc"]} == with_ws


def test_every_size_helper_belongs_to_a_row_and_every_row_names_an_export():
    helpers = {n for n in header_functions() if n.endswith("_workspace_bytes")}
    named = {r["helper"] for r in wc.ROWS}
    assert len(helpers) >= 13
    assert named == helpers, (sorted(named - helpers), sorted(helpers - named))
    # the helper is the entry's own: same stem, or the one helper two entries share
    for r in wc.ROWS:
        stem = r["helper"][:-len("_workspace_bytes")]
        assert r["entry"].startswith(stem) or r["helper"] == "tspn_stem_bf16_workspace_bytes", r["entry"]


def test_caller_zeroed_scratch_is_what_the_header_says():
    fns = header_functions()
    for entry, param, what, tests in wc.CALLER_ZEROED:
        assert re.search(r"\b%s\b" % param, fns[entry]) and what and tests, entry
    text = open(HEADER).read()
    assert "zeroed\n *   by the caller" in text and "one zeroed byte per" in text


def test_other_scratch_is_what_the_header_says(tspn):
    fns = header_functions()
    lib = tspn._abi.lib()
    for entry, param, helper, tests in wc.OTHER_SCRATCH:
        assert re.search(r"\bvoid\s*\*\s*%s\b" % param, fns[entry]) and helper in fns and tests, entry
        assert not re.search(r"\bvoid\s*\*\s*workspace\b", fns[entry]) and not helper.endswith("_workspace_bytes"), entry
    assert [c[0] for c in wc.OTHER_SCRATCH] == ["tspn_heads_pairgrid_f16x3"]
    split_bytes = lib.tspn_heads_pairgrid_f16x3_split_bytes
    assert split_bytes(64, 12) == 256 + 2 * 2048 and split_bytes(32, 1) == split_bytes(32, 16) == 256 + 2048
    assert split_bytes(48, 12) == 0 and split_bytes(64, 17) == 0          # a C and an H the entry refuses
    assert "every byte of\n * which the call writes before it reads it" in open(HEADER).read()


def test_every_named_test_exists():
    defined = {}
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        tree = ast.parse(open(path).read(), filename=path)
        defined[f"tests/{os.path.basename(path)}"] = {
            n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test")}
    missing = []
    for entry, nodes in ([(r["entry"], r["tests"]) for r in wc.ROWS] + [(c[0], c[3]) for c in wc.CALLER_ZEROED] +
                         [(c[0], c[3]) for c in wc.OTHER_SCRATCH]):
        for node in nodes:
            path, _, name = node.partition("::")
            if name.split("[")[0] not in defined.get(path, ()):
                missing.append(f"{entry}: {node}")
    assert not missing, "rows name tests that do not exist:\n" + "\n".join(missing)


def test_the_library_memsets_the_table_lists_are_in_the_sources():
    """The rows that say "library: hipMemsetAsync ..." name memsets that exist; a memset added to an entry's file without
    a word in the table fails here too."""
    csrc = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd", "csrc")
    count = {}
    for path in glob.glob(os.path.join(csrc, "**", "*.hip"), recursive=True):
        n = len(re.findall(r"\bhipMemsetAsync\s*\(", open(path).read()))
        if n:
            count[os.path.basename(path)] = n
    assert count == {"tspn_fused.hip": 2, "tspn_bf16.hip": 1, "tspn_pairlist_bf16.hip": 1}
    listed = " ".join(r["zeroed"] for r in wc.ROWS)
    for name in count:
        assert name in listed, f"{name} clears scratch, the table does not say so"


# ---------------------------------------------------------------------------------------------- helper against entry
_raw = ctypes.create_string_buffer(4096 + 256)
PTR = (ctypes.addressof(_raw) + 255) // 256 * 256       # every operand: non-null, 256-byte aligned, never read


def _fused(tspn, shape):
    d = tspn._abi.FusedDesc()
    d.B, d.N, d.T, d.D, d.A, d.K, d.P, d.conv_algo = shape
    d.canonical_pairs = 0
    for f in ("feats", "pairs", "conv_packed", "conv_bias", "head_w", "head_b", "cls_w", "cls_b", "out_heads", "out_logits"):
        setattr(d, f, PTR)
    return d


def _fused_bf16(tspn, shape):
    d = tspn._abi.FusedBf16Desc()
    d.B, d.N, d.T, d.D, d.A, d.K, d.P = shape
    for f in ("feats", "pairs", "conv_packed", "conv_bias", "head_packed", "head_b", "cls_w", "cls_b", "out_heads",
              "out_logits"):
        setattr(d, f, PTR)
    return d


def _call_fused(fn):
    def call(tspn, lib, shape, ws, nbytes):
        d = _fused(tspn, shape)
        d.workspace, d.workspace_bytes = ws, nbytes
        return getattr(lib, fn)(ctypes.byref(d), None)
    return call


def _call_fused_bf16(fn):
    def call(tspn, lib, shape, ws, nbytes):
        d = _fused_bf16(tspn, shape)
        d.workspace, d.workspace_bytes = ws, nbytes
        return getattr(lib, fn)(ctypes.byref(d), None)
    return call


# entry -> (helper(tspn, lib, shape), call(tspn, lib, shape, ws, nbytes), shapes that run, shapes the entry refuses)
P_ = PTR
PROBES = {
    "tspn_predicate_head_f32": (
        lambda tspn, lib, s: lib.tspn_predicate_head_workspace_bytes(*s),
        lambda tspn, lib, s, ws, n: lib.tspn_predicate_head_f32(P_, s[0], s[1], s[1], P_, P_, s[2], P_, 1, ws, n, None),
        [(65, 257, 145), (200, 1001, 132), (992, 11070, 132), (1, 3, 1)],       # (P, F, K)
        [(4, 0, 3), (4, 8, 0), (-1, 8, 3)]),
    "tspn_predicate_head_norm_f32": (
        lambda tspn, lib, s: lib.tspn_predicate_head_norm_workspace_bytes(*s),
        lambda tspn, lib, s, ws, n: lib.tspn_predicate_head_norm_f32(P_, s[0], s[1], s[1], P_, P_, s[2], s[3], s[4], s[5],
                                                                     P_, 1, ws, n, None),
        [(3, 40, 5, 4, 6, 5), (200, 1001, 17, 1, 250, 4), (992, 11070, 132, 70, 1000, 8)],   # (P, F, K, first, block, nblocks)
        [(4, 8, 3, 4, 3, 2), (4, 8, 3, -1, 3, 2), (4, 8, 3, 0, 0, 2), (4, 0, 3, 0, 1, 0)]),
    "tspn_conv3_tc_wino63_f32": (
        lambda tspn, lib, s: lib.tspn_conv3_tc_wino63_workspace_bytes(s[0], s[1], s[2]),
        lambda tspn, lib, s, ws, n: lib.tspn_conv3_tc_wino63_f32(P_, s[0], s[1], s[2], P_, s[3], P_, 0, P_, ws, n, None),
        [(3, 7, 32, 32), (27, 31, 32, 640), (512, 150, 2048, 8192)],            # (B, T, Cin, M)
        [(3, 7, 16, 32), (3, 0, 32, 32), (3, 7, 0, 32), (-1, 7, 32, 32)]),
    "tspn_conv3_tc_wino63_f16x3": (
        lambda tspn, lib, s: lib.tspn_conv3_tc_wino63_f16x3_workspace_bytes(*s),
        lambda tspn, lib, s, ws, n: lib.tspn_conv3_tc_wino63_f16x3(P_, s[0], s[1], s[2], P_, s[3], P_, 0, P_, ws, n, None),
        [(3, 7, 64, 256), (40, 149, 64, 512), (512, 150, 2048, 8192)],
        [(3, 7, 64, 128), (3, 7, 48, 256), (3, 0, 64, 256), (-1, 7, 64, 256)]),
    "tspn_decode_topk_f32": (
        lambda tspn, lib, s: lib.tspn_decode_topk_workspace_bytes(s[0], s[1], min(s[3], s[2])),
        lambda tspn, lib, s, ws, n: lib.tspn_decode_topk_f32(P_, P_, P_, P_, 40, s[1], 1, s[0], s[1], s[2], 35, s[3], 200,
                                                             P_, P_, P_, ws, n, None),
        [(3, 56, 132, 20), (1, 2, 5, 20), (2, 992, 132, 20)],                   # (S, P, K, topk_pair)
        [(3, 56, 132, 0), (3, 56, 132, -2)]),
    "tspn_forward_fused_f32": (
        lambda tspn, lib, s: lib.tspn_forward_fused_workspace_bytes(ctypes.byref(_fused(tspn, s))),
        _call_fused("tspn_forward_fused_f32"),
        [(1, 8, 30, 16, 4, 132, 56, 0), (3, 5, 33, 18, 4, 132, 60, 0), (2, 6, 149, 32, 4, 7, 60, 1),
         (1, 9, 7, 64, 4, 132, 72, 2), (16, 32, 150, 2048, 4, 132, 15872, 2)],  # (B, N, T, D, A, K, P, conv_algo)
        [(1, 8, 30, 16, 6, 132, 56, 0), (1, 8, 0, 16, 4, 132, 56, 0), (1, 8, 30, 16, 4, 0, 56, 0), (1, 8, 30, 16, 0, 132, 56, 0)]),
    "tspn_forward_fused_bf16": (
        lambda tspn, lib, s: lib.tspn_forward_fused_bf16_workspace_bytes(ctypes.byref(_fused_bf16(tspn, s))),
        _call_fused_bf16("tspn_forward_fused_bf16"),
        [(1, 17, 7, 16, 4, 132, 272), (2, 16, 30, 32, 4, 9, 480), (1, 64, 900, 1024, 4, 132, 4032)],   # (B, N, T, D, A, K, P)
        [(1, 17, 7, 24, 4, 132, 272), (1, 17, 7, 16, 6, 132, 272), (1, 17, 0, 16, 4, 132, 272), (1, 17, 7, 16, 0, 132, 272)]),
    "tspn_forward_fused_bf16_pairs": (
        lambda tspn, lib, s: lib.tspn_forward_fused_bf16_pairs_workspace_bytes(ctypes.byref(_fused_bf16(tspn, s))),
        _call_fused_bf16("tspn_forward_fused_bf16_pairs"),
        [(1, 17, 7, 16, 4, 132, 5), (2, 16, 30, 32, 4, 9, 1000), (1, 64, 900, 1024, 4, 132, 4032)],
        [(1, 2049, 7, 16, 4, 132, 5), (1, 17, 7, 24, 4, 132, 5), (1, 17, 7, 16, 6, 132, 5), (1, 17, 7, 16, 4, 132, 2 ** 31)]),
    "tspn_heads_pairlist_bf16": (
        lambda tspn, lib, s: lib.tspn_heads_pairlist_bf16_workspace_bytes(s[0], s[1], s[2]),
        lambda tspn, lib, s, ws, n: lib.tspn_heads_pairlist_bf16(P_, 64, s[0], s[1], 32, 18, P_, s[2], P_, P_, 12, P_, ws, n,
                                                                 None),
        [(1, 5, 1), (2, 17, 300), (1, 2048, 7)],                                # (B, N, P)
        [(1, 2049, 7), (1, 17, 2 ** 31), (1, 17, -1)]),
    "tspn_span_predicate_f32": (
        lambda tspn, lib, s: lib.tspn_span_predicate_workspace_bytes(*s),
        lambda tspn, lib, s, ws, n: lib.tspn_span_predicate_f32(P_, s[0], s[1], s[2], P_, P_, 40, P_, P_, s[3], P_, ws, n,
                                                                None),
        [(3, 1, 16, 3), (4, 9, 40, 145), (32, 150, 2048, 132)],                 # (NT, T, D, K)
        [(3, 0, 16, 3), (3, 9, 0, 3), (3, 9, 16, 0)]),
    "tspn_decode_span_relations_f32": (
        lambda tspn, lib, s: lib.tspn_decode_span_relations_workspace_bytes(*s),
        lambda tspn, lib, s, ws, n: lib.tspn_decode_span_relations_f32(P_, s[0], s[1], s[2], s[3], P_, s[4], P_, P_, P_, s[5],
                                                                       P_, P_, s[6], P_, 35, s[7], 200, P_, P_, P_, P_, P_, P_,
                                                                       ws, n, None),
        [(1, 2, 1, 16, 2, 1, 1, 1), (3, 5, 12, 32, 20, 4, 132, 20), (2, 6, 9, 16, 30, 16, 145, 256)],   # (S,N,T,D,P,J,K,R)
        [(3, 5, 12, 32, 20, 17, 132, 20), (3, 5, 12, 32, 20, 4, 257, 20), (3, 5, 0, 32, 20, 4, 132, 20),
         (3, 5, 12, 32, 20, 4, 132, 0)]),
    "tspn_span_predicate_bf16": (
        lambda tspn, lib, s: lib.tspn_span_predicate_bf16_workspace_bytes(*s),
        lambda tspn, lib, s, ws, n: lib.tspn_span_predicate_bf16(P_, s[0], s[1], s[2], P_, P_, s[4], P_, P_, s[3], P_, ws, n,
                                                                 None),
        [(3, 1, 16, 3, 40), (4, 9, 48, 145, 33), (64, 900, 1024, 132, 16128)],  # (NT, T, D, K, P)
        [(4, 9, 24, 5, 3), (4, 0, 16, 5, 3), (4, 9, 16, 0, 3)]),
    "tspn_decode_span_relations_bf16": (
        lambda tspn, lib, s: lib.tspn_decode_span_relations_bf16_workspace_bytes(*s),
        lambda tspn, lib, s, ws, n: lib.tspn_decode_span_relations_bf16(P_, s[0], s[1], s[2], s[3], P_, s[4], P_, P_, P_, s[5],
                                                                        P_, P_, s[6], P_, 35, s[7], 200, P_, P_, P_, P_, P_,
                                                                        P_, ws, n, None),
        [(1, 2, 1, 16, 2, 1, 1, 1), (3, 5, 12, 32, 20, 4, 132, 20), (2, 6, 9, 16, 30, 16, 145, 256)],
        [(3, 5, 12, 32, 20, 17, 132, 20), (3, 5, 12, 24, 20, 4, 132, 20), (3, 5, 0, 32, 20, 4, 132, 20),
         (3, 5, 12, 32, 20, 4, 132, 0)]),
    "tspn_stem_conv_bf16": (
        lambda tspn, lib, s: lib.tspn_stem_bf16_workspace_bytes(*s),
        lambda tspn, lib, s, ws, n: lib.tspn_stem_conv_bf16(P_, s[0], s[1], s[2], P_, 64, P_, ws, n, P_, None),
        [(1, 7, 7), (2, 30, 41), (8, 720, 1280)],                               # (NB, H, W)
        [(1, 0, 7), (1, 7, -1), (-1, 7, 7)]),
    "tspn_stem_pool_bf16": (
        lambda tspn, lib, s: lib.tspn_stem_bf16_workspace_bytes(*s),
        lambda tspn, lib, s, ws, n: lib.tspn_stem_pool_bf16(P_, s[0], s[1], s[2], P_, 32, P_, ws, n, P_, None),
        [(1, 7, 7), (2, 30, 41), (8, 720, 1280)],
        [(1, 0, 7), (1, 7, -1), (-1, 7, 7)]),
}


def test_every_row_has_a_probe():
    assert set(PROBES) == {r["entry"] for r in wc.ROWS}


@pytest.mark.parametrize("entry", sorted(PROBES))
def test_helper_and_entry_agree_without_a_device(tspn, entry):
    lib = tspn._abi.lib()
    helper, call, shapes, _ = PROBES[entry]
    for s in shapes:
        need = helper(tspn, lib, s)
        assert need > 0, f"{entry}{s}: the helper returns 0 for a shape the entry serves"
        rc = call(tspn, lib, s, PTR, 0)
        msg = lib.tspn_last_error().decode()
        assert rc == tspn._abi.TSPN_EWORKSPACE, f"{entry}{s}: a workspace of 0 bytes gave {rc} ({msg})"
        m = re.search(r"workspace 0 < (\d+) bytes", msg)
        assert m, f"{entry}{s}: the refusal does not say what it needs: {msg!r}"
        assert int(m.group(1)) == need, f"{entry}{s}: the helper says {need} bytes, the entry wants {m.group(1)}"
        # no workspace at all is refused as well, before anything is read
        rc = call(tspn, lib, s, None, need)
        assert rc in (tspn._abi.TSPN_EWORKSPACE, tspn._abi.TSPN_EINVAL), f"{entry}{s}: a null workspace gave {rc}"


@pytest.mark.parametrize("entry", sorted(PROBES))
def test_helper_returns_zero_for_the_shapes_the_entry_refuses(tspn, entry):
    lib = tspn._abi.lib()
    helper, call, _, refused = PROBES[entry]
    assert refused
    for s in refused:
        rc = call(tspn, lib, s, PTR, 0)          # the shape is looked at before the workspace: not TSPN_EWORKSPACE
        assert rc in (tspn._abi.TSPN_EINVAL, tspn._abi.TSPN_EUNSUPPORTED), \
            f"{entry}{s}: expected a refusal of the shape, got {rc} ({lib.tspn_last_error().decode()})"
        assert helper(tspn, lib, s) == 0, f"{entry}{s}: refused with {rc}, but the helper asks for {helper(tspn, lib, s)} bytes"
