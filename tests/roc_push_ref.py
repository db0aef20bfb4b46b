"""The id push of the k_roc_encode_u2 dense step in Python: a port of csrc/u2_push_ref.h (checked against it by
tests/test_u2_push_cpu.py), and the encode of a whole list with both forms side by side, which gives every step's push class and the
copy of the unrolled loop it runs in.

classes: 0 C (no spill), 1 A (slice 0 spills), 2 B (slice 1 spills), 3 both (the two-slice form only; never seen)."""
import numpy as np

L = 1 << 31
C, A, B, BOTH = 0, 1, 2, 3
M64 = (1 << 64) - 1
SAFE_HI = 0x7FF80000  # U2_SAFE_HI
RING_ROOM = 48        # U2_RING_ROOM


def push_widths(P):
    """(p0, p1) of precision P: codec.cpp:92-105"""
    return min(P, 16), (min(P - 16, 16) if P > 16 else 0)


def push_two(q, x, p0, p1):
    """codec.cpp:65-76 for the two slices -> (head, words pushed, class)"""
    words, cls = [], 0
    head = q
    if head >= ((L >> p0) << 32):
        words.append(head & 0xFFFFFFFF)
        head >>= 32
        cls |= A
    head = ((head << p0) + (x & 0xFFFF)) & M64
    if head >= ((L >> p1) << 32):
        words.append(head & 0xFFFFFFFF)
        head >>= 32
        cls |= B
    head = ((head << p1) + (x >> 16)) & M64
    return head, words, cls


def push_class(q, p0, p1):
    return A if q >= 1 << (63 - p0) else B if q >= 1 << (63 - p0 - p1) else C


def push_one(q, x, p0, p1):
    """u2_push_one: the class from q, then B, the multiplier of x_lo, the spilled word -> (head, B, mul, words pushed, class)"""
    cls = push_class(q, p0, p1)
    x_lo, x_hi = x & 0xFFFF, x >> 16
    if cls == C:
        Bv, mul, words = (q << (p0 + p1)) & M64, 1 << p1, []
    elif cls == A:
        Bv, mul, words = ((q >> 32) << (p0 + p1)) & M64, 1 << p1, [q & 0xFFFFFFFF]
    else:
        Bv, mul, words = ((q >> (32 - p0)) << p1) & M64, 0, [((q << p0) & 0xFFFFFFFF) | x_lo]
    return (Bv + x_lo * mul + x_hi) & M64, Bv, mul, words, cls


def needs_generic(head):
    """u2_needs_generic (roc_u2.h): the index pop of this head may renormalise"""
    return (head >> 31) == 0 or (head >> 32) >= SAFE_HI


def classify_encode(order, P, mt_table=(), copies=8):
    """Encode the ids `order` (the oracle's sampling order: order[i] is the id of step i) at precision P as codec.cpp:131-137 does,
    with both forms of the push side by side, and follow k_roc_encode_u2's dense loop through it: which steps run in the unrolled
    loop (the others are generic steps of the C++ glue), in which of its `copies` copies, and where it leaves for a ring spill.
    A pop from the empty stack takes mt_table[draws] (codec.h:32-40; mt_table = Oracle.mt_table(count)).
    -> dict(cls = class of every step, copy = copy of every step (-1: generic step), classes = steps per class, by_copy[copy][class],
            spill_after = class of the last loop step in front of each ring spill of U2_ENC_OUTER, blocks = divisor block changes,
            head, words, mt_draws)"""
    p0, p1 = push_widths(P)
    n = len(order)
    st, head, draws = [], L, 0
    cls_of = np.zeros(n, np.uint8)
    copy_of = np.full(n, -1, np.int8)
    by_copy = np.zeros((copies, 3), np.int64)
    spill_after, blocks = [], 0
    lo = 0            # ring: words [lo, sp) are resident, sp = len(st)
    in_loop = False   # inside the asm statement; t, t_end, left as s69, s70, s86; c = the copy the next step runs in
    t = t_end = left = c = 0
    for i in range(n):
        nmax = n - i
        x = int(order[i])
        assert x >> P == 0, "the id does not fit the precision (reference carry quirk: not a chain list)"
        if not in_loop:
            if len(st) - lo >= RING_ROOM:
                lo += 32
            if nmax >= 3 and not needs_generic(head):
                in_loop, t, left, c = True, 0, nmax - 2, 0
                t_end = min(left, 63)
            elif len(st) - lo < 8 and lo:  # ws_prepare of the generic step
                lo -= 32
        # index pop, codec.cpp:21-42
        h = head
        if h >= nmax * ((L // nmax) << 32):
            assert not in_loop, "the loop's exit test let a renormalising index pop through"
            st.append(h & 0xFFFFFFFF)
            h >>= 32
        q = h // nmax
        if h < L:
            assert not in_loop
            if st:
                w = st.pop()
            else:
                w = int(mt_table[draws])
                draws += 1
            q = w | (q << 32)
        assert 1 <= q < 1 << 63
        h2, w2, c2 = push_two(q, x, p0, p1)
        h1, Bv, mul, w1, c1 = push_one(q, x, p0, p1)
        assert c2 != BOTH and len(w2) <= 1, f"step {i}: two spills"
        assert (h1, w1, c1) == (h2, w2, c2), f"step {i}: the two forms differ on q {q:#x}, x {x:#x}"
        st.extend(w2)
        head = h2
        assert head < 1 << 63  # slices 2 and 3 (precision 0) never spill behind a P-bit id
        cls_of[i] = c1
        if not in_loop:
            continue
        copy_of[i] = c
        by_copy[c, c1] += 1
        # the tail of the step: exit tests on B, ring test in the last copy
        ok = (Bv >> 31) != 0 and (Bv >> 32) < SAFE_HI
        lim = t_end if ok else 0
        if c == copies - 1 and len(st) - lo >= RING_ROOM:
            lim = 0
        t += 1
        if t < lim:
            c = (c + 1) % copies
            continue
        # U2_ENC_OUTER
        if len(st) - lo >= RING_ROOM:
            lo += 32
            spill_after.append(int(c1))
        if t >= 63:
            blocks += 1
            left -= 63
            t, t_end = 0, min(left, 63)
        if t < t_end and ok:
            c = 0
        else:
            in_loop = False
    classes = [int((cls_of == k).sum()) for k in (C, A, B)]
    return dict(cls=cls_of, copy=copy_of, classes=classes, by_copy=by_copy, spill_after=spill_after, blocks=blocks,
                head=head, words=np.array(st, dtype=np.uint32), mt_draws=draws)
