// shard_plan.h -- the host part of vidc_shards (include/vidc.h): which shard owns which list, the lists' local numbers and offsets, the
// segment tables of the cut, the routing of requests and the byte layout of the scratch blocks.  Host code only, no HIP include:
// tests/shard_plan_test.cpp, shard_plan_owner_test.cpp and shard_blocks_test.cpp build it with g++.
//
// Ownership is the longest-processing-time rule on the list lengths, stated so that it equals sharding.lpt_partition bit for bit: lists
// are taken in descending size, ties by ascending list number; each goes to the shard with the least load so far, ties to the lowest
// shard number.  The local number of a list is its rank among its owner's lists in ascending global number.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

namespace vidc {
namespace shardplan {

// one run of a segmented copy, in elements: dst[dst_start .. dst_start + count) = src[src_start .. src_start + count)
struct Segment {
    uint64_t src_start, dst_start, count;
};
// a wavefront's share of a segment: elements [start, start + SHARD_COPY_UNIT) of segment `seg`
struct CopyChunk {
    uint32_t seg, start;
};
constexpr uint32_t SHARD_COPY_UNIT = 1024;

struct ShardPlan {
    int nshards = 0;
    uint64_t nlist = 0, ntotal = 0;
    std::vector<uint64_t> offsets;                     // the caller's CSR offsets, nlist + 1
    std::vector<int32_t> owner;                        // per list
    std::vector<uint32_t> local_no;                    // per list
    std::vector<uint64_t> load;                        // per shard: ids
    std::vector<std::vector<uint64_t>> lists;          // per shard: its lists' global numbers, ascending
    std::vector<std::vector<uint64_t>> local_offsets;  // per shard: CSR offsets of its lists, lists[s].size() + 1
    std::vector<std::vector<Segment>> cut;             // per shard: one segment per non-empty list, src = global ids, dst = the shard's ids
    uint64_t size_of(uint64_t list) const { return offsets[list + 1] - offsets[list]; }
    // the device form of the map: shard << 32 | local_no
    uint64_t packed(uint64_t list) const { return (uint64_t)(uint32_t)owner[list] << 32 | local_no[list]; }
};

// owner[l] by the LPT rule (sizes[l] = length of list l)
inline std::vector<int32_t> lpt_partition(const std::vector<uint64_t> &sizes, int nshards) {
    std::vector<int32_t> owner(sizes.size(), 0);
    if (nshards <= 1 || sizes.empty()) return owner;
    std::vector<uint64_t> order(sizes.size());
    std::iota(order.begin(), order.end(), (uint64_t)0);
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return sizes[a] > sizes[b]; });
    std::vector<uint64_t> load((size_t)nshards, 0);
    for (uint64_t l : order) {
        int best = 0;
        for (int s = 1; s < nshards; s++)
            if (load[(size_t)s] < load[(size_t)best]) best = s;  // (strict: ties stay with the lowest shard)
        owner[l] = best;
        load[(size_t)best] += sizes[l];
    }
    return owner;
}

// The plan of a GIVEN ownership (owner[l] in 0 .. nshards - 1; the caller checked): local numbers, local offsets, loads and cut segments.
// An append keeps the owner of every list and re-plans with the new offsets: the local numbers depend on the owner alone, so they stay.
// offsets: nlist + 1 entries, offsets[0] == 0, monotone (the caller checked)
inline ShardPlan make_plan_for_owner(const uint64_t *offsets, uint64_t nlist, int nshards, std::vector<int32_t> owner) {
    ShardPlan p;
    p.nshards = nshards;
    p.nlist = nlist;
    p.offsets.assign(offsets, offsets + nlist + 1);
    p.ntotal = offsets[nlist];
    p.owner = std::move(owner);
    p.local_no.assign(nlist, 0);
    p.load.assign((size_t)nshards, 0);
    p.lists.assign((size_t)nshards, {});
    p.local_offsets.assign((size_t)nshards, std::vector<uint64_t>(1, 0));
    p.cut.assign((size_t)nshards, {});
    for (uint64_t l = 0; l < nlist; l++) {
        const size_t s = (size_t)p.owner[l];
        p.local_no[l] = (uint32_t)p.lists[s].size();
        p.lists[s].push_back(l);
        const uint64_t n = offsets[l + 1] - offsets[l];
        if (n) p.cut[s].push_back(Segment{offsets[l], p.local_offsets[s].back(), n});
        p.local_offsets[s].push_back(p.local_offsets[s].back() + n);
        p.load[s] += n;
    }
    return p;
}

// the plan of vidc_shards_encode: ownership by the LPT rule, the rest from it
inline ShardPlan make_plan(const uint64_t *offsets, uint64_t nlist, int nshards) {
    std::vector<uint64_t> sizes(nlist);
    for (uint64_t l = 0; l < nlist; l++) sizes[l] = offsets[l + 1] - offsets[l];
    return make_plan_for_owner(offsets, nlist, nshards, lpt_partition(sizes, nshards));
}

// vidc_rebalance_sharded: the lists of one object under two maps.  Per NEW shard one row per local list, in local order: the list is
// local list list_no[j] of OLD shard src_no[j] -- the table vidc_roc_regroup takes, with the old shard objects as its sources.
struct RegroupRows {
    std::vector<uint32_t> src_no;
    std::vector<uint64_t> list_no;
};
// old_p, new_p: plans of the same offsets over the same number of shards (the caller made new_p from old_p.offsets)
inline std::vector<RegroupRows> regroup_plan(const ShardPlan &old_p, const ShardPlan &new_p) {
    std::vector<RegroupRows> rows((size_t)new_p.nshards);
    for (size_t d = 0; d < rows.size(); d++) {
        rows[d].src_no.reserve(new_p.lists[d].size());
        rows[d].list_no.reserve(new_p.lists[d].size());
        for (uint64_t l : new_p.lists[d]) {
            rows[d].src_no.push_back((uint32_t)old_p.owner[l]);
            rows[d].list_no.push_back(old_p.local_no[l]);
        }
    }
    return rows;
}
// the ids whose owner changes between the two maps
inline uint64_t moved_ids(const ShardPlan &old_p, const ShardPlan &new_p) {
    uint64_t moved = 0;
    for (uint64_t l = 0; l < old_p.nlist; l++)
        if (old_p.owner[l] != new_p.owner[l]) moved += old_p.size_of(l);
    return moved;
}

// the chunk table of a segment table: every segment cut into pieces of SHARD_COPY_UNIT elements (lists are Zipf: one wavefront per
// list would leave a 52 k-id list to one wavefront next to hundreds that copy one id)
inline std::vector<CopyChunk> build_copy_chunks(const std::vector<Segment> &segs) {
    std::vector<CopyChunk> c;
    uint64_t total = 0;
    for (const Segment &s : segs) total += s.count;
    c.reserve(segs.size() + total / SHARD_COPY_UNIT);
    for (size_t i = 0; i < segs.size(); i++)
        for (uint64_t st = 0; st < segs[i].count; st += SHARD_COPY_UNIT) c.push_back(CopyChunk{(uint32_t)i, (uint32_t)st});
    return c;
}

// vidc_shards_decode_lists: request order and repeats are kept.  Per shard: the local numbers of its requested lists (in request
// order) and the segments that put its decoded lists (back to back in the shard's staging) where the request wants them.
struct ListsRoute {
    std::vector<uint64_t> out_offsets;               // m + 1
    std::vector<std::vector<uint64_t>> local_lists;  // per shard
    std::vector<std::vector<Segment>> place;         // per shard: src = the shard's staging, dst = the caller's output
    std::vector<uint64_t> staged;                    // per shard: ids in its staging
};
// false: a list number >= nlist (*bad = its position in the request)
inline bool route_lists(const ShardPlan &p, uint64_t m, const uint64_t *list_nos, ListsRoute &r, uint64_t *bad) {
    r.out_offsets.assign(m + 1, 0);
    r.local_lists.assign((size_t)p.nshards, {});
    r.place.assign((size_t)p.nshards, {});
    r.staged.assign((size_t)p.nshards, 0);
    for (uint64_t i = 0; i < m; i++) {
        const uint64_t l = list_nos[i];
        if (l >= p.nlist) {
            if (bad) *bad = i;
            return false;
        }
        const size_t s = (size_t)p.owner[l];
        const uint64_t n = p.size_of(l);
        r.local_lists[s].push_back(p.local_no[l]);
        if (n) r.place[s].push_back(Segment{r.staged[s], r.out_offsets[i], n});
        r.staged[s] += n;
        r.out_offsets[i + 1] = r.out_offsets[i] + n;
    }
    return true;
}

// vidc_shards_decode_gather: every mention of a list becomes a slot of its owner's request, every item goes to the owner of its slot.
struct GatherRoute {
    std::vector<std::vector<uint64_t>> local_lists, item_slot, item_off, item_index;  // per shard; item_index: place in ids_out
};
// 0: routed.  1: a list number >= nlist, 2: an item outside its list (*bad = its position)
inline int route_gather(const ShardPlan &p, uint64_t m, const uint64_t *list_nos, uint64_t n_items, const uint64_t *item_slot,
                        const uint64_t *item_off, GatherRoute &r, uint64_t *bad) {
    const size_t ns = (size_t)p.nshards;
    r.local_lists.assign(ns, {});
    r.item_slot.assign(ns, {});
    r.item_off.assign(ns, {});
    r.item_index.assign(ns, {});
    std::vector<uint64_t> slot_local(m);
    for (uint64_t i = 0; i < m; i++) {
        const uint64_t l = list_nos[i];
        if (l >= p.nlist) {
            if (bad) *bad = i;
            return 1;
        }
        const size_t s = (size_t)p.owner[l];
        slot_local[i] = r.local_lists[s].size();
        r.local_lists[s].push_back(p.local_no[l]);
    }
    for (uint64_t i = 0; i < n_items; i++) {
        if (item_slot[i] >= m || item_off[i] >= p.size_of(list_nos[item_slot[i]])) {
            if (bad) *bad = i;
            return 2;
        }
        const size_t s = (size_t)p.owner[list_nos[item_slot[i]]];
        r.item_slot[s].push_back(slot_local[item_slot[i]]);
        r.item_off[s].push_back(item_off[i]);
        r.item_index[s].push_back(i);
    }
    return 0;
}

// The byte offsets of the two scratch blocks of a routed call (translate_labels, append, remove) over n requests.  A section the call
// does not have is empty.  The 8-byte sections come first, so they are 8-aligned; a mask starts at a multiple of 16 (the byte inverse
// cut takes its 16-byte path by the alignment of both runs) and has its length rounded up to 16; 16 bytes of slack end a block.
//   home block:               invalid[ns] | local[ns * n] | answers[ns * n] | the shards' masks | found[ns * n] bytes | owner[n] bytes
//   a far shard's own block:  invalid, 16 bytes | local[n] | ids[n] | answers[n] | found[n] bytes | its mask
struct UpdateBlocks {
    size_t local = 0, answers = 0, found = 0, owner = 0, total = 0, found_bytes = 0;  // home block: shard i's slice of a section is its i-th n
    size_t f_local = 0, f_ids = 0, f_answers = 0, f_found = 0, f_mask = 0;            // a far shard's block
    std::vector<size_t> mask, f_total;                                                // per shard: its mask in the home block, its far block's size
};
// mask_len: per shard, or NULL for a call without masks
inline UpdateBlocks update_blocks(uint32_t nshards, uint64_t n, bool has_local, bool has_answers, const uint64_t *mask_len, bool has_found,
                                  bool has_owner) {
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t ns = nshards;
    UpdateBlocks b;
    b.local = ns * 8;
    b.answers = b.local + (has_local ? ns * n * 8 : 0);
    b.found = up16(b.answers + (has_answers ? ns * n * 8 : 0));
    b.f_local = 16;
    b.f_ids = b.f_local + (has_local ? n * 8 : 0);
    b.f_answers = b.f_ids + n * 8;
    b.f_found = b.f_answers + (has_answers ? n * 8 : 0);
    b.f_mask = up16(b.f_found + (has_found ? n : 0));
    for (size_t i = 0; i < ns; i++) {
        const size_t len = up16(mask_len ? mask_len[i] : 0);
        b.mask.push_back(b.found);  // (found follows the last mask)
        b.found += len;
        b.f_total.push_back(b.f_mask + len + 16);
    }
    b.found_bytes = has_found ? ns * n : 0;
    b.owner = b.found + b.found_bytes;
    b.total = b.owner + (has_owner ? n : 0) + 16;
    return b;
}

}  // namespace shardplan
}  // namespace vidc
