"""The slot -> object map of the split-fp16 pair stage (csrc/pairf16/tspn_heads_pair_f16x3.hip) as plain arithmetic, no
GPU.  Wave w of a tile is subject w.  In a diagonal tile (subject block == object block) it walks seven slots, slot i =
object (w + 1 + i) & 7, and never object w; in every other tile eight slots, slot i = object i.  The kernel's walk and its
epilogue must use the same map, so the expression is looked up in the source in both places."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "temporal-span-proposal-network-vidvrd_amd", "csrc", "pairf16", "tspn_heads_pair_f16x3.hip")
PF_O = 8


def slots(diag):
    return PF_O - 1 if diag else PF_O


def slot_object(w, i, diag):
    return (w + 1 + i) & 7 if diag else i


def test_diagonal_walk_is_a_permutation_of_the_other_objects():
    for w in range(PF_O):
        walk = [slot_object(w, i, True) for i in range(slots(True))]
        assert sorted(walk) == [o for o in range(PF_O) if o != w], (w, walk)
        assert walk[0] == (w + 1) % PF_O and all((b - a) % PF_O == 1 for a, b in zip(walk, walk[1:]))


def test_off_diagonal_walk_is_the_identity():
    for w in range(PF_O):
        assert [slot_object(w, i, False) for i in range(slots(False))] == list(range(PF_O))


def test_every_pair_of_a_diagonal_tile_has_exactly_one_slot():
    owner = {}
    for w in range(PF_O):
        for i in range(slots(True)):
            assert owner.setdefault((w, slot_object(w, i, True)), i) == i
    assert set(owner) == {(s, o) for s in range(PF_O) for o in range(PF_O) if s != o}


def test_the_kernel_uses_this_map_in_its_walk_and_in_its_epilogue():
    src = re.sub(r"//[^\n]*", "", open(SRC).read())
    walk = re.search(r"DIAG \? \(\(wave \+ 1 \+ i\) & 7\) : i", src)
    store = re.search(r"diag \? \(wave \+ 1 \+ o\) & 7 : o", src)
    assert walk and store, "the slot -> object expression of the walk or of the epilogue changed: update this file with it"
    assert re.search(r"NS = DIAG \? PF_O - 1 : PF_O", src) and re.search(r"diag && o == PF_O - 1\) continue", src)
    assert re.search(r"const bool diag = diag_skip && sb == ob;", src)
