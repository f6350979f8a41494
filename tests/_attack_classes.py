"""The classes of position that the attack set (targets() in knightvision_amd/csrc/kv_movegen.h, the reference's
squareUnderAttack) special-cases, told from a state vector and its recorded 64-bit attack set alone. Shared by
tests/golden/make_golden.py (--attacks-only), which asserts that tests/golden/attacks.npz holds every class, and by
the tests that compare against that fixture. Not a test module itself.

The attacker is the side NOT to move; bit r * 8 + c of the set is squareUnderAttack(r, c). Codes: 1..6 white
K Q R B N p, 7..12 black K Q R B N p."""
import os

import numpy as np

CLASSES = ("ep_beside", "castle_w_king", "castle_w_queen", "castle_b_king", "castle_b_queen", "double_free",
           "double_blocked", "diag_empty_not_attacked", "push_attacks", "pawn_file_a", "pawn_file_h")


def classes_of(v, att):
    """The classes state vector `v` (80 int8) with attack set `att` (int) holds, as a set of names."""
    att = int(att)
    out = set()
    white = int(v[64]) == 0  # the attacker's colour: the side not to move
    pawn = 6 if white else 12
    ma, start = (-1, 6) if white else (1, 1)
    ep = None if v[75] < 0 else (int(v[75]), int(v[76]))

    def at(r, c):
        return int(v[r * 8 + c])

    def bit(r, c):
        return (att >> (r * 8 + c)) & 1

    for r in range(8):
        for c in range(8):
            if at(r, c) != pawn or not 0 <= r + ma < 8:
                continue
            if c == 0:
                out.add("pawn_file_a")
            if c == 7:
                out.add("pawn_file_h")
            if at(r + ma, c) == 0:
                if bit(r + ma, c):
                    out.add("push_attacks")
                if r == start:
                    if at(r + 2 * ma, c) == 0 and bit(r + 2 * ma, c):
                        out.add("double_free")
                    if at(r + 2 * ma, c) != 0:
                        out.add("double_blocked")
            for dc in (-1, 1):
                if not 0 <= c + dc < 8:
                    continue
                if (r + ma, c + dc) == ep and at(r + ma, c + dc) == 0 and bit(r + ma, c + dc):
                    out.add("ep_beside")
                elif at(r + ma, c + dc) == 0 and not bit(r + ma, c + dc):
                    out.add("diag_empty_not_attacked")  # and no other piece of the attacker reaches it
    # castle destinations: the attacker's king at home and unmoved, the rook unmoved and in its corner, the
    # squares between them empty -- the nested probes return False, so nothing else is asked
    row = 7 if white else 0
    k_moved, rk_moved, rq_moved = (v[69], v[71], v[72]) if white else (v[70], v[73], v[74])
    king, rook = (1, 3) if white else (7, 9)
    kr, kc = (int(v[65]), int(v[66])) if white else (int(v[67]), int(v[68]))
    if (kr, kc) == (row, 4) and at(row, 4) == king and not k_moved:
        tag = "w" if white else "b"
        if not rk_moved and at(row, 5) == 0 and at(row, 6) == 0 and at(row, 7) == rook and bit(row, 6):
            out.add(f"castle_{tag}_king")
        if not rq_moved and at(row, 1) == 0 and at(row, 2) == 0 and at(row, 3) == 0 and at(row, 0) == rook \
                and bit(row, 2):
            out.add(f"castle_{tag}_queen")
    return out


def count_classes(states, att):
    """{class: the number of states that hold it}."""
    counts = {name: 0 for name in CLASSES}
    for v, a in zip(states, att):
        for name in classes_of(v, a):
            counts[name] += 1
    return counts


# ---- the fixture: (file of the states, its key, the key of their attack sets in attacks.npz)
SETS = (("movegen", "states", "movegen_pre"), ("movegen", "post_states", "movegen_post"),
        ("movegen_wide", "states", "movegen_wide_pre"), ("movegen_wide", "post_states", "movegen_wide_post"))


def recorded(golden_dir):
    """[(name of the set, states [n, 80], the reference's attack sets [n] uint64)]."""
    att = np.load(os.path.join(golden_dir, "attacks.npz"))
    assert sorted(att.files) == sorted(k for _, _, k in SETS)
    out = []
    for name, key, akey in SETS:
        states = np.ascontiguousarray(np.load(os.path.join(golden_dir, name + ".npz"))[key])
        assert att[akey].dtype == np.uint64 and att[akey].shape == (len(states),)
        out.append((akey, states, att[akey]))
    return out


def differing(got, want):
    """The states whose sets differ, and the bits that differ in the first of them."""
    bad = np.flatnonzero(got != want)
    first = [s for s in range(64) if (int(got[bad[0]]) ^ int(want[bad[0]])) >> s & 1] if len(bad) else []
    return bad.tolist()[:5], len(bad), first
