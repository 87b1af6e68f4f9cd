"""The tree checker (tests/_tree_ref.py) on a six-entry tree written out by
hand: child order, flags, rollups, the digests' messages and top_rep. No GPU."""
import struct

import numpy as np
import pytest

from tests import _tree_ref as R
from tests._oracle import load_oracle


def _name(first, last=0):
    b = np.zeros(32, np.uint8)
    b[0], b[31] = first, last
    return b


#   0 A/            2 files, one empty directory
#   1 A/x   10 B    name 02..
#   2 A/y    5 B    name 01..   (orders before x)
#   3 B/            one invalid file: incomplete
#   4 B/z    7 B    invalid
#   5 A/e/          name 03.., empty
PARENT = [-1, 0, 0, -1, 3, 0]
IS_DIR = [1, 0, 0, 1, 0, 1]
NAMES = np.stack([_name(9), _name(2), _name(1), _name(8), _name(1), _name(3)])
SIZES = [0, 10, 5, 0, 7, 0]
VALID = [0, 1, 1, 0, 0, 0]


def _digests():
    d = np.zeros((6, 32), np.uint8)
    d[1], d[2], d[4] = 0x11, 0x22, 0x44
    return d


def test_plan_of_the_hand_made_tree():
    depth, children, levels = R.tree_plan(PARENT, IS_DIR)
    assert depth.tolist() == [0, 1, 1, 0, 1, 1] and children.tolist() == [3, 0, 0, 1, 0, 0] and levels == 2
    for parent, is_dir, code in (([1, 0], [1, 1], R.INVALID), ([0], [1], R.INVALID), ([-1, 0], [0, 0], R.INVALID),
                                 ([2, -1], [1, 1], R.INVALID), ([-2], [1], R.INVALID)):
        with pytest.raises(R.ShapeError) as e:
            R.tree_plan(parent, is_dir)
        assert e.value.code == code


def test_digests_of_the_hand_made_tree():
    oracle = load_oracle()
    kids, _ = R.child_order(PARENT, NAMES)
    assert kids == [[2, 1, 5], [], [], [4], [], []]
    r = R.tree_digests(oracle, PARENT, IS_DIR, NAMES, _digests(), VALID, SIZES)
    assert r["flags"].tolist() == [R.DIR, 0, 0, R.DIR | R.INCOMPLETE, 0, R.DIR | R.EMPTY]
    assert r["tree_bytes"].tolist() == [15, 10, 5, 7, 7, 0] and r["tree_files"].tolist() == [2, 1, 1, 1, 1, 0]
    assert r["valid"].tolist() == [1, 1, 1, 0, 0, 0]
    assert r["counts"] == {"entries": 6, "dirs": 3, "complete_dirs": 2, "empty_dirs": 1, "levels": 2,
                           "largest_dir": 3}
    t_e = oracle.hash(b"SDTREE01" + struct.pack("<Q", 0))
    assert r["T"][5] == t_e and 3 not in r["T"]
    rec = lambda nm, content, kind: nm.tobytes() + content + struct.pack("<Q", kind)
    m_a = b"SDTREE01" + struct.pack("<Q", 3) + rec(NAMES[2], b"\x22" * 32, 0) + rec(NAMES[1], b"\x11" * 32, 0) + \
        rec(NAMES[5], bytes.fromhex(t_e), 1)
    assert len(m_a) == 16 + 72 * 3 and r["T"][0] == oracle.hash(m_a)
    assert bytes(r["digests"][0]).hex() == r["T"][0] and int(r["keys"][0]) == int(r["T"][0][:16], 16)
    assert not r["digests"][3].any() and r["keys"][3] == 0
    # the file entries' slots are as they were
    assert (r["digests"][[1, 2, 4]] == _digests()[[1, 2, 4]]).all()
    # equal name32: index order; a NULL valid: every file takes part
    names = NAMES.copy()
    names[1] = names[2]
    assert R.child_order(PARENT, names)[0][0] == [1, 2, 5]
    assert R.tree_digests(oracle, PARENT, IS_DIR, NAMES, _digests())["flags"][3] == R.DIR


def test_top_of_the_hand_made_tree():
    # A and B carry one label, x and y another: both of those lie inside A
    top, flags, counts = R.tree_top(PARENT, [0, 1, 1, 0, -1, 5])
    assert top.tolist() == [0, -1, -1, 0, -1, -1]
    assert flags.tolist() == [R.DUP, R.DUP | R.NESTED, R.DUP | R.NESTED, R.DUP, 0, 0]
    assert counts == {"entries": 5, "dup_entries": 4, "nested_entries": 2, "top_entries": 2, "kept_classes": 1,
                      "dropped_classes": 1}
    # z, moved to the root, joins x and y's class from outside any duplicate directory: kept whole
    top, flags, counts = R.tree_top([-1, 0, 0, -1, -1, 0], [0, 1, 1, 0, 1, 5])
    assert top.tolist() == [0, 1, 1, 0, 1, -1] and flags.tolist() == [1, 3, 3, 1, 1, 0]
    assert counts == {"entries": 6, "dup_entries": 5, "nested_entries": 2, "top_entries": 5, "kept_classes": 2,
                      "dropped_classes": 0}
    # a stray label takes no part; a stray parent is a root in the device form
    top, flags, _ = R.tree_top([7, 0], [1, 1], stray_parent_is_root=True)
    assert top.tolist() == [1, 1] and flags.tolist() == [1, 3]
    assert R.tree_top([-1, -1], [2, -7])[0].tolist() == [-1, -1]
