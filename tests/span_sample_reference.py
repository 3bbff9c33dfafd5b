"""Numpy restatement of the span anchor sampler (DESIGN.md 2 "span anchor sampling"), written from the rules there: the words
of hashrng.bits, a shift, a stable argsort of (key, index) within each class, the quotas; the generators of label vectors and
the case list of tests/test_gpu_span_sample.py, whose conditions tests/test_span_sample_host.py checks without a GPU.

The device gets hashrng.stream_key(seed, tag); the restatement gets (seed, tag) and goes through hashrng.bits itself, so the
two sides share nothing but the definition of the stream."""
import functools

import numpy as np

from tspn_mi355x import hashrng

CHUNK = 4096                  # anchors per workgroup of the kernels (tests/spansample_kernel_variants.py)
OFFSET_THREADS = 256          # threads of the one-workgroup offsets kernel: more chunks than that = several per thread
FULL_N = 992 * 4 * 150        # a cfg2 segment: P A T = 595 200 anchors


def rounds_of(key_bits):
    return (key_bits + 7) // 8


def keys_ref(seed, tag, n, key_bits):
    """key(i) uint64 [n] = word i of stream (seed, tag) shifted down to key_bits bits."""
    return hashrng.bits(seed, tag, n) >> np.uint64(64 - key_bits)


def quotas_ref(n_pos, n_neg, batch, want_pos):
    sel_pos = min(n_pos, want_pos)
    return sel_pos, min(n_neg, batch - sel_pos)


def sample_ref(label, seed, tag, key_bits, batch, want_pos):
    """(mask uint8 of label's shape, counts int64 [4] = (n_pos, n_neg, sel_pos, sel_neg), info) of one segment.
    info[c] for class c (0 positive, 1 negative) with sel > 0: threshold key, the class's threshold-equal anchors (flat
    indices, ascending), how many of them are taken, and the radix round that decides the threshold (below)."""
    label = np.asarray(label)
    flat = label.reshape(-1)
    n = flat.size
    key = keys_ref(seed, tag, n, key_bits)
    members = [np.flatnonzero(flat >= 1), np.flatnonzero(flat == 0)]
    sel = quotas_ref(len(members[0]), len(members[1]), batch, want_pos)
    mask = np.zeros(n, np.uint8)
    info = {}
    for c in (0, 1):
        m = members[c]                                              # ascending flat index: a stable sort orders by (key, i)
        order = np.argsort(key[m], kind="stable")
        mask[m[order[:sel[c]]]] = 1
        if sel[c] > 0:
            thr = key[m[order[sel[c] - 1]]]
            equal = m[key[m] == thr]
            info[c] = {"threshold": int(thr), "equal": equal, "taken": int(mask[equal].sum()),
                       "decided_round": decided_round(key[m], thr, key_bits)}
    return mask.reshape(label.shape), np.array([len(members[0]), len(members[1]), sel[0], sel[1]], np.int64), info


def decided_round(class_keys, thr, key_bits):
    """The first radix round (8-bit digits, most significant first, the last digit at bit 0) after which the anchors that
    share their digits so far with the threshold all equal it: the round in which the search for it ends."""
    R = rounds_of(key_bits)
    for r in range(R):
        shift = np.uint64(8 * (R - 1 - r))
        under = class_keys[(class_keys >> shift) == (np.uint64(thr) >> shift)]
        if (under == np.uint64(thr)).all():
            return r
    raise AssertionError("the last round compares whole keys")


def regime(counts, batch, want_pos):
    """The quota regime of a case, as a name."""
    n_pos, n_neg, sel_pos, sel_neg = (int(v) for v in counts)
    if batch == 0:
        return "empty batch"
    if n_pos == 0 and n_neg == 0:
        return "nothing to select"
    if n_pos == want_pos and want_pos > 0:
        return "positives exactly the quota"
    if sel_pos + sel_neg < batch:
        return "both classes short: all taken"
    if n_pos < want_pos:
        return "positives short: negatives fill"
    return "both quotas bind"


# --------------------------------------------------------------------------------------------------------- generators
MIXES = ("mixed", "no_pos", "no_neg", "only_ignored", "few_pos", "one_pos", "both_short", "exact_pos")


def make_labels(seed, n, mix, want_pos=128):
    """label int8 [n].  Positives are 1 and a few 2s, ignored anchors -1 and a few -128 (the class rule is >= 1, == 0, < 0).
      mixed         2 % positive, 10 % ignored, the rest negative
      no_pos        10 % ignored, the rest negative          no_neg      half positive, half ignored
      only_ignored  all negative labels                      few_pos     5 positives (or n // 2), the rest negative
      one_pos       1 positive, the rest negative            both_short  20 positives and 30 negatives (or n // 3 each),
      exact_pos     min(want_pos, n) positives, rest negative            the rest ignored"""
    assert mix in MIXES, mix
    u = hashrng.integers(seed, f"labels/{mix}", (n,), 0, 1000)
    where = np.argsort(hashrng.bits(seed, f"places/{mix}", n), kind="stable")     # a fixed shuffle of the indices
    label = np.zeros(n, np.int64)
    if mix == "mixed":
        label = np.where(u < 20, 1, np.where(u < 120, -1, 0))
    elif mix == "no_pos":
        label = np.where(u < 100, -1, 0)
    elif mix == "no_neg":
        label = np.where(u < 500, 1, -1)
    elif mix == "only_ignored":
        label[:] = -1
    elif mix in ("few_pos", "one_pos"):
        label[where[:min(5 if mix == "few_pos" else 1, n // 2)]] = 1
    elif mix == "both_short":
        label[:] = -1
        k = min(20, n // 3)
        label[where[:k]] = 1
        label[where[k:k + min(30, n // 3)]] = 0
    elif mix == "exact_pos":
        label[where[:min(want_pos, n)]] = 1
    v = hashrng.integers(seed, f"values/{mix}", (n,), 0, 8)
    label = np.where((label == 1) & (v == 0), 2, np.where((label == -1) & (v == 0), -128, label))
    return label.astype(np.int8)


# ---------------------------------------------------------------------------------------------------------- the cases
def _case(n, key_bits, mix="mixed", batch=256, fraction=0.5, seed=0, name=None):
    return {"id": name or f"n{n}-k{key_bits}-{mix}-b{batch}-f{fraction}", "n": n, "key_bits": key_bits, "mix": mix,
            "batch": batch, "fraction": fraction, "seed": seed}


SIZES = (1, 63, 64, 65, 1023, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, (OFFSET_THREADS + 1) * CHUNK + 3)
KEY_BITS = (1, 4, 8, 9, 16, 17, 32)
MID = 3 * CHUNK + 5


def _cases():
    out = []
    for n in SIZES:                                     # around one wave, one chunk, several chunks, several chunks a thread
        out += [_case(n, 32), _case(n, 4)]
    out += [_case(MID, kb) for kb in KEY_BITS]          # 1 .. 4 rounds; heavy ties on the threshold at 1 and 4 bits
    for mix in MIXES:
        out += [_case(MID, 8, mix), _case(MID, 17, mix), _case(MID, 32, mix)]
    out += [_case(5 * CHUNK + 77, 9, "one_pos"), _case(5 * CHUNK + 77, 16, "few_pos")]
    for batch in (0, 1, 256):
        out += [_case(MID, 16, "mixed", batch, f) for f in (0.0, 0.5, 1.0)]
    seen, uniq = set(), []
    for c in out:
        if c["id"] not in seen:
            seen.add(c["id"])
            uniq.append(c)
    return uniq


CASES = _cases()


def tag_of(case):
    return f"span_sample_test/{case['id']}"


def want_pos_of(case):
    return int(case["batch"] * case["fraction"])


def batch_on_a_close_pair(label, seed, tag, key_bits, shift):
    """A batch (with want_pos = 0: negatives only) whose threshold is the FIRST, in (key, index) order, of two negatives
    whose keys agree above bit `shift`: with shift = 8 the search for the threshold is decided in the last of four rounds,
    with shift = 0 the two keys are equal and the tie rule decides between them.  None if the labels hold no such pair."""
    flat = np.asarray(label).reshape(-1)
    m = np.flatnonzero(flat == 0)
    key = keys_ref(seed, tag, flat.size, key_bits)[m]
    order = np.argsort(key, kind="stable")
    top = key[order] >> np.uint64(shift)
    same = np.flatnonzero(top[1:] == top[:-1])
    return None if same.size == 0 else int(same[0]) + 1


@functools.lru_cache(maxsize=None)
def special_cases():
    """(case, label) of the two constructed cases: the threshold decided in round 3 of 4, and the full cfg2 size with the
    threshold between two anchors of equal 32-bit keys."""
    out = []
    for name, n, shift in (("last-round", MID, 8), ("full-size-tie", FULL_N, 0)):
        case = _case(n, 32, "mixed", 0, 0.0, seed=5, name=name)
        label = make_labels(case["seed"], n, "mixed")
        case["batch"] = batch_on_a_close_pair(label, case["seed"], tag_of(case), 32, shift)
        label.setflags(write=False)
        out.append((case, label))
    return out


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """(case, label, mask, counts, info) of one case, computed once and shared; never written to."""
    for case, label in [(c, None) for c in CASES] + list(special_cases()):
        if case["id"] == case_id:
            break
    else:
        raise KeyError(case_id)
    if label is None:
        label = make_labels(case["seed"], case["n"], case["mix"], want_pos_of(case))
        label.setflags(write=False)
    mask, counts, info = sample_ref(label, case["seed"], tag_of(case), case["key_bits"], case["batch"], want_pos_of(case))
    mask.setflags(write=False)
    counts.setflags(write=False)
    return case, label, mask, counts, info


ALL_IDS = [c["id"] for c in CASES] + ["last-round", "full-size-tie"]
