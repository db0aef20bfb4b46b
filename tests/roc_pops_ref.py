"""The slice pops of the k_roc_decode_u2 step in Python: a port of csrc/u2_pops_ref.h (checked against it by
tests/test_u2_pops_cpu.py), and the decode of a whole stream with them, which gives every step's refill class.

classes: 0 none, 1 slice-0 refill, 2 slice-1 refill, 3 both (the two-pop form only; never seen for a head >= 2^31)."""
import bisect

import numpy as np

L = 1 << 31
NONE, SLICE0, SLICE1, BOTH = 0, 1, 2, 3
M64 = (1 << 64) - 1


def pop_widths(P):
    """(p1, p0) of precision P: codec.cpp:107-121"""
    return (min(P - 16, 16) if P > 16 else 0), min(P, 16)


def pops_two(head, p1, p0, pop):
    """codec.cpp:78-90 for the two slices; pop() returns the next stack word -> (head, x, popped, class)"""
    cls = popped = 0
    x_hi = head & ((1 << p1) - 1)
    head >>= p1
    if head < L:
        head = (head << 32) | pop()
        popped += 1
        cls |= SLICE1
    x_lo = head & ((1 << p0) - 1)
    head >>= p0
    if head < L:
        head = (head << 32) | pop()
        popped += 1
        cls |= SLICE0
    return head, (x_hi << 16) | x_lo, popped, cls


def pops_one(head, w, p1, p0):
    """U2_DEC_TOP_P / U2_DEC_SIDE_P (u2_pops_one): one test of head', one shift, at most one refill with the word w"""
    lo = head & 0xffffffff
    m1, m0 = (1 << p1) - 1, (1 << p0) - 1
    if head >> (31 + p1):
        x_hi = lo & m1
        x_lo = (lo >> p1) & m0 if p0 else 0  # s_bfe_u32, offset p1, width p0
        head >>= p1 + p0
        if head >> 31:
            return head, (x_hi << 16) | x_lo, 0, NONE
        return ((head & 0xffffffff) << 32) | w, (x_hi << 16) | x_lo, 1, SLICE0
    x_hi = lo & m1
    head >>= p1
    head = ((head & 0xffffffff) << 32) | w
    x_lo = w & m0
    return head >> p0, (x_hi << 16) | x_lo, 1, SLICE1


def classify_decode(head, words, n, P, want_ids=None, mt_draws=0, mt_table=()):
    """Decode n ids of precision P from (head, words) as codec.cpp:140-152 does, with both forms of the pops side by side.
    want_ids: the oracle's decode in sampling order (out[n - 1 - i] is the id of step i); every step's id is compared with it.
    A pop from the empty stack takes mt_table[mt_draws] and counts it (codec.h:32-40; mt_table = Oracle.mt_table(count)).
    Only streams that decode to a set (ranks by bisection).
    -> dict(classes=[steps per class], undone=slice-0 refills whose word the index push put back, slice1_after_renorm, max_popped)"""
    p1, p0 = pop_widths(P)
    st = [int(w) for w in np.asarray(words)]
    head = int(head)
    seen = []
    classes = [0, 0, 0, 0]
    undone = slice1_after = max_popped = 0
    renorm_before = False
    draws = [int(mt_draws)]

    def pop():
        if st:
            return st.pop()
        draws[0] += 1
        return int(mt_table[draws[0] - 1])

    for i in range(n):
        assert head >= L, "the head fell below 2^31"
        w = st[-1] if st else int(mt_table[draws[0]])  # (the fast loop is never entered on an empty ring; the model takes the draw)
        one = pops_one(head, w, p1, p0)
        two = pops_two(head, p1, p0, pop)
        assert one == two, f"step {i}: the two forms differ on head {head:#x}: {one} / {two}"
        head, x, popped, cls = two
        classes[cls] += 1
        max_popped = max(max_popped, popped)
        if cls == SLICE1 and renorm_before:
            slice1_after += 1
        if want_ids is not None:
            assert x == int(want_ids[n - 1 - i]), f"step {i}: id {x}, the oracle has {int(want_ids[n - 1 - i])}"
        rank = bisect.bisect_left(seen, x)
        assert rank == len(seen) or seen[rank] != x, "multiset stream"
        seen.insert(rank, x)
        nmax = i + 1
        renorm_before = False
        if head >= ((L // nmax) << 32):  # codec.cpp:44-63
            st.append(head & 0xffffffff)
            if cls == SLICE0:
                assert st[-1] == w
                undone += 1
            head >>= 32
            renorm_before = True
        head = head * nmax + rank
        if head < L:
            head = pop() | (head << 32)
    return dict(classes=classes, undone=undone, slice1_after_renorm=slice1_after, max_popped=max_popped, end_head=head, end_words=len(st), mt_draws=draws[0])
