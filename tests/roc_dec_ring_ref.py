"""The ring traffic of the k_roc_decode_u2 step in Python: a port of csrc/u2_dec_ring_ref.h (checked against it by
tests/test_u2_dec_ring_cpu.py), and the decode of a whole stream with both forms side by side, which gives every step's class.

classes: 0 quiet (the ring, sp and the carried word stay), 1 refill only, 2 spill only (h_hi >= lq: never reached while nmax <= 2^P),
3 the slice-1 side path."""
import bisect

import numpy as np

from roc_pops_ref import L, SLICE1, pop_widths, pops_one

QUIET, REFILL, SPILL, SIDE = 0, 1, 2, 3
NAMES = ("quiet", "refill only", "spill only", "side")


def ring_lq(nmax):
    return L // nmax


def ring_class(h, lq):
    """the class of a common-path step from h = head' >> (p1 + p0) and lq alone"""
    return REFILL if h < lq else SPILL if (h >> 32) >= lq else QUIET


def _push(head, lq, ring, sp):
    """index push, first half (codec.cpp:44-63 as the step runs it) -> (H, sp, carried word, slot, word)"""
    lo, hi = head & 0xffffffff, head >> 32
    slot = sp & 63
    ring[slot] = lo
    if hi >= lq:
        H, sp = hi, sp + 1
    else:
        H = head
    return H, sp, ring[(sp - 1) & 63], slot, lo


def dec_ring_ref(head, sp, ring, lq, p1, p0):
    """u2_dec_ring_ref: pops_one, then the push; ring is a list of 64 words and is changed in place
    -> (cls, H, x, sp, w, wrote, slot, word)"""
    head, x, popped, pcls = pops_one(head, ring[(sp - 1) & 63], p1, p0)
    sp0 = sp - popped
    H, sp, w, slot, word = _push(head, lq, ring, sp0)
    spilled = sp != sp0
    cls = SIDE if pcls == SLICE1 else QUIET if (popped == 1) == spilled else SPILL if spilled else REFILL
    return cls, H, x, sp, w, 1, slot, word


def dec_ring_cls(head, sp, ring, w, lq, p1, p0):
    """u2_dec_ring_cls: one class out of (h, lq); quiet steps touch nothing -> (cls, H, x, sp, w, wrote, slot, word)"""
    lo = head & 0xffffffff
    m1, m0 = (1 << p1) - 1, (1 << p0) - 1
    x_hi = lo & m1
    if head >> (31 + p1):
        x_lo = (lo >> p1) & m0 if p0 else 0
        h = head >> (p1 + p0)
        t = 0xffffffff if h < lq else h >> 32
        if t < lq:
            return QUIET, h, (x_hi << 16) | x_lo, sp, w, 0, 0, 0
        if h >> 31:
            cls = SPILL
        else:
            cls, h, sp = REFILL, ((h & 0xffffffff) << 32) | w, sp - 1
    else:
        h = ((((head >> p1) & 0xffffffff) << 32) | w) >> p0
        x_lo = w & m0
        cls, sp = SIDE, sp - 1
    H, sp, w, slot, word = _push(h, lq, ring, sp)
    return cls, H, (x_hi << 16) | x_lo, sp, w, 1, slot, word


def classify_decode(head, words, n, P, want_ids=None, mt_draws=0, mt_table=(), rank="set", entry_bits=6):
    """Decode n ids of precision P from (head, words) as codec.cpp:140-152 does, every step with both forms of the ring traffic on
    rings of their own (the whole stack is kept beside them, so the 64 slots hold the top words as the kernel's ring does).
    want_ids: the oracle's decode in sampling order (out[n - 1 - i] is the id of step i); every step's id is compared with it.
    Multiset streams are fine: the rank is the number of strictly smaller ids decoded so far (fenwick_tree.h:42-94).
    A step whose head falls below 2^31 behind the index push is followed by the generic second half (a pop), as the kernel's exit is.
    rank="bitmap": the rank as k_roc_decode_u2 computes it, from counters that count every decoded id and a bitmap that holds an id
    once: ids below x's level-2 entry (2^entry_bits ids: 6 for the one-word steps, 8 for the four-word step) with their multiplicity
    plus the DISTINCT ids of the entry below x.  On a set that is the rank; on a multiset stream it is smaller from the first
    duplicate on, so the kernel's first pass over such a stream (the one the recount throws away) sees other heads than the oracle's
    decode does: this mode follows the kernel's, and want_ids has no meaning for it.
    -> dict(cls=array of n classes, generic_after=array of n bools (head < 2^31 behind the step's index push), counts=[4],
            sp_before=n + 1 stack sizes in front of every step (and behind the last), sp_mid=n stack sizes behind the first half of
            every step's index push (in front of the pop that generic_after marks))"""
    p1, p0 = pop_widths(P)
    st = [int(w) for w in np.asarray(words)]
    draws = [int(mt_draws)]
    head = int(head)
    seen = []
    cls_of = np.zeros(n, np.int8)
    generic_after = np.zeros(n, bool)
    sp_before = np.zeros(n + 1, np.int64)
    sp_mid = np.zeros(n, np.int64)
    assert rank in ("set", "bitmap") and (rank == "set" or want_ids is None)
    below_entry = np.zeros((1 << max(P - entry_bits, 0)) + 1, np.int64)  # bitmap rank: decoded ids per entry, with multiplicity
    distinct = set()

    def ring_of():
        """the 64 ring slots from the stack's top words; below an empty stack, the draws the pops would take"""
        r = [0] * 64
        sp = len(st)
        for k in range(1, min(sp, 64) + 1):
            r[(sp - k) & 63] = st[sp - k]
        return r

    for i in range(n):
        assert head >= L, "the head fell below 2^31"
        nmax = i + 1
        lq = ring_lq(nmax)
        sp_before[i] = len(st)
        drew = not st
        if drew:  # (the fast loop never runs on an empty ring; the model lends the stack the word a pop would draw, codec.h:32-40)
            st.append(int(mt_table[draws[0]]))
        sp = len(st)
        ra, rb = ring_of(), ring_of()
        a = dec_ring_ref(head, sp, ra, lq, p1, p0)
        b = dec_ring_cls(head, sp, rb, rb[(sp - 1) & 63], lq, p1, p0)
        assert a[:5] == b[:5], f"step {i}: the two forms differ on head {head:#x}, nmax {nmax}: {a} / {b}"
        cls, H, x, nsp, w = b[:5]
        assert w == rb[(nsp - 1) & 63]
        for k in range(1, min(nsp, 60) + 1):
            assert ra[(nsp - k) & 63] == rb[(nsp - k) & 63], f"step {i}: the rings differ below sp"
        common = head >> (31 + p1) != 0
        if common:
            assert cls == ring_class(head >> (p1 + p0), lq)
        popped = cls in (REFILL, SIDE) or (cls == QUIET and (head >> (p1 + p0)) < L)
        if nsp > sp:
            st.append(ra[sp & 63])  # a spill-only step adds its word; every other class leaves the words below min(sp, nsp) alone
        elif nsp < sp:
            st.pop()
        if drew:
            if popped:
                draws[0] += 1       # the lent word was drawn (and, in a quiet step, pushed back)
            else:
                del st[0]
        assert len(st) == nsp - (1 if drew and not popped else 0)
        cls_of[i] = cls
        sp_mid[i] = len(st)
        if want_ids is not None:
            assert x == int(want_ids[n - 1 - i]), f"step {i}: id {x}, the oracle has {int(want_ids[n - 1 - i])}"
        if rank == "set":
            r = bisect.bisect_left(seen, x)
            seen.insert(r, x)
        else:
            e, e0 = x >> entry_bits, (x >> entry_bits) << entry_bits
            r = int(below_entry[:e].sum()) + sum(1 for y in range(e0, x) if y in distinct)
            below_entry[e] += 1
            distinct.add(x)
        head = H * nmax + r
        if head < L:
            generic_after[i] = True
            if st:
                head = st.pop() | (head << 32)
            else:
                head = int(mt_table[draws[0]]) | (head << 32)
                draws[0] += 1
    sp_before[n] = len(st)
    return dict(cls=cls_of, generic_after=generic_after, counts=np.bincount(cls_of, minlength=4).tolist(), end_head=head,
                end_words=len(st), mt_draws=draws[0], sp_before=sp_before, sp_mid=sp_mid, distinct=len(distinct))


RING_LO, RING_HI = 18, 53  # U2_DEC_RING_LO, U2_DEC_RING_HI


def kernel_walk(m, n, nwords):
    """Which code of k_roc_decode_u2 runs every step of a decode that classify_decode stepped through (m): the while loop of the
    kernel with its ring glue (csrc/roc_u2.h) and the control of the eight-copy loop (U2_DEC_BOT_NR_U, U2_DEC_BOT_T_U,
    U2_DEC_OUTER_TR), on the stack sizes of m.  lo is the first ring-resident word as WStack keeps it (csrc/wave.h).
      * top of the while loop: more than 56 words in the ring spill 32, fewer than 22 with words below refill 32; then a generic
        step unless 18 .. 53 words are in the ring (a generic step's ws_prepare spills above 56 and refills below 8);
      * the asm is entered at copy 0 with t = 0 and a block of min(steps left, 64) steps (U2_DEC_ENTRY_U: both carried scalars
        loaded); every copy goes on while head' >= 2^31 and t < the block's end, copy 7 also only while the ring holds 18 .. 53
        words; behind copy 7 of t = 64 the block changes (t = 0, the re-entry of U2_DEC_OUTER_U loads both scalars again) and the
        loop goes on unless head' < 2^31, the ring test failed or the list is done; behind an exit through head' < 2^31 the C++ code
        runs the second half of the index push (ws_prepare, a pop).
    -> dict(path=n (0 generic step, 1 the loop), copy=n (-1 outside the loop), entry_first / block_first=n bools (the step is the
            first behind U2_DEC_ENTRY_U / behind a block change inside the asm), behind_generic=n bools (an entry_first step whose
            predecessor was a generic step), ring_exits (ways out of the asm through the ring test), lo_moves)"""
    cls, hlt, spb, spm = m["cls"], m["generic_after"], m["sp_before"], m["sp_mid"]
    path = np.zeros(n, np.int8)
    copy = np.full(n, -1, np.int8)
    entry_first = np.zeros(n, bool)
    block_first = np.zeros(n, bool)
    behind_generic = np.zeros(n, bool)
    lo = ((int(nwords) - 1) & ~31) if nwords else 0
    ring_exits = lo_moves = 0
    i = 0

    def ring_ok(sp):
        return RING_LO <= sp - lo <= RING_HI

    while i < n:
        res = int(spb[i]) - lo
        if res > 56:
            lo, lo_moves = lo + 32, lo_moves + 1
        elif res < 22 and lo:
            lo, lo_moves = lo - 32, lo_moves + 1
        if not ring_ok(int(spb[i])):
            res = int(spb[i]) - lo  # the generic step's ws_prepare
            if res > 56:
                lo, lo_moves = lo + 32, lo_moves + 1
            elif res < 8 and lo:
                lo, lo_moves = lo - 32, lo_moves + 1
            i += 1
            continue
        assert int(spb[i]) - lo <= 64
        entry_first[i] = True
        behind_generic[i] = i > 0 and path[i - 1] == 0
        t, left = 0, n - i
        t_end = min(left, 64)
        while True:
            path[i], copy[i] = 1, t % 8
            below = hlt[i]
            sp = int(spm[i])
            assert 0 < sp - lo <= 64, "the ring over- or underflowed inside the loop"
            i, t = i + 1, t + 1
            if not below and t < t_end and (t % 8 or ring_ok(sp)):
                continue
            out = below or not ring_ok(sp)
            if t == 64:
                t, left = 0, left - 64
                t_end = min(left, 64)
            if t >= t_end or out:
                ring_exits += int(out and not below and i < n)
                break
            block_first[i] = True
        if below:  # the second half of the last index push: ws_prepare, then the pop
            res = int(spm[i - 1]) - lo
            if res > 56:
                lo, lo_moves = lo + 32, lo_moves + 1
            elif res < 8 and lo:
                lo, lo_moves = lo - 32, lo_moves + 1
    return dict(path=path, copy=copy, entry_first=entry_first, block_first=block_first, behind_generic=behind_generic,
                ring_exits=ring_exits, lo_moves=lo_moves)
