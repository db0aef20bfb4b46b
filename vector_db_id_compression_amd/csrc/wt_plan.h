// wt_plan.h -- the deciding half of the wavelet tree's host calls (wt.hip): the constants the kernels share, the geometry of an object
// (levels, words, rank blocks, RRR blocks and samples, the element count of every device array), the shape verdict, the offset-stream
// bases, the image word counts and the two size formulas -- each once, for build, import, image_words and export_all --, the build's
// choice between the partitioned and the direct scatter with every grid and scratch count, the grids and scratch of decode_all and of
// the import's rebuild passes, and the host checks of an image (wt_image_check).  Host code with no HIP include and nothing that
// touches a stream: tests/wt_plan_test.cpp builds it with g++.  wt.hip fills WtBuildPolicy from the environment and the context.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#ifndef VIDC_HD
#ifdef __HIPCC__
#define VIDC_HD __host__ __device__
#else
#define VIDC_HD
#endif
#endif

// ---- the partitioned scatter (k_wt_part_*): (id, list) pairs by id >> 14 into <= 1024 buckets, 1024 workgroups over the positions
#define VIDC_WTP_BSH 14u
#define VIDC_WTP_BUCKET (1u << VIDC_WTP_BSH)
#define VIDC_WTP_MAXB 1024u  // buckets
#define VIDC_WTP_NBLK 1024u  // workgroups of the two passes over the positions (16 384 positions each at 16.8 M ids)
#define VIDC_WTP_MIN_IDS (1ull << 18)    // the partitioned scatter is built for 2^18 <= ntotal <= 2^24 ids ...
#define VIDC_WTP_MAX_IDS (1ull << 24)    // (<= 1024 buckets of 2^14 ids)
#define VIDC_WTP_MAX_LISTS (1ull << 18)  // ... and <= 2^18 lists (the list number shares a dword with 14 id bits)
// ---- one level of the build in one pass (k_wt_level)
#define VIDC_WT_EPT 64u                    // elements per thread
#define VIDC_WT_TILE (256u * VIDC_WT_EPT)  // 16 384 positions = 256 bit-vector words = 32 rank blocks per workgroup
#define VIDC_WT_NR_G 16u                   // workgroups per level of k_wt_node_ranks_from_C
// ---- one level of the bulk decode (k_wt_decode_tile): tiles of 8192 positions
#define VIDC_WTD_EPT 32u

namespace vidc {
namespace dev {

constexpr uint32_t BLK_WORDS = 8;  // 512-bit rank blocks
constexpr uint32_t RRR_B = 63, RRR_K = 32;  // bits per RRR block, blocks per sample
VIDC_HD inline uint64_t wt_nrank_base(uint32_t level) { return ((uint64_t)1 << level) - 1u + level; }  // sum of (2^j + 1), j < level
VIDC_HD inline uint64_t wtp_chunk(uint64_t ntotal) {  // positions per workgroup: whole 4096-position tiles
    return ((ntotal + VIDC_WTP_NBLK - 1u) / VIDC_WTP_NBLK + 4095u) & ~4095ull;
}

}  // namespace dev

// ---- shape: what build and import accept
constexpr uint64_t WT_NLIST_END = 0xffffffffull, WT_NTOTAL_END = 0xffffffffull;  // nlist in 1 .. 2^32 - 2, ntotal < 2^32 - 1
enum WtShape { WT_SHAPE_OK, WT_SHAPE_TYPE /* wt_type is not 0 or 1 */, WT_SHAPE_NLIST, WT_SHAPE_NTOTAL };
inline bool wt_ntotal_ok(uint64_t ntotal) { return ntotal < WT_NTOTAL_END; }
inline WtShape wt_shape_check(uint64_t nlist, uint64_t ntotal, int wt_type) {
    if (wt_type != 0 && wt_type != 1) return WT_SHAPE_TYPE;
    if (nlist == 0 || nlist >= WT_NLIST_END) return WT_SHAPE_NLIST;
    return wt_ntotal_ok(ntotal) ? WT_SHAPE_OK : WT_SHAPE_NTOTAL;
}
// L = max(1, bit_width(nlist - 1)): the smallest L >= 1 with 2^L >= nlist.  An accepted nlist is below 2^32, so L <= 32 -- no
// refusal of "more than 32 levels" exists, and the off_base[32] a kernel's RRR view carries (rrr_view) holds every level.
inline uint32_t wt_levels(uint64_t nlist) {
    uint32_t L = 1;
    while ((1ull << L) < nlist) L++;
    return L;
}

inline uint64_t wt_words(uint64_t bits) { return (bits + 63) / 64; }

// ---- geometry of an object of an accepted shape
struct WtGeom {
    int wt_type;
    uint32_t L;
    uint64_t ntotal;
    uint64_t W;                 // words of a level's bits in an image: ceil(ntotal / 64)
    uint64_t words_per_level;   // as stored: W + one pad word (two-word reads)
    uint64_t blocks_per_level;  // 512-bit rank blocks of the stored words
    uint64_t nblk, nsamp;       // RRR blocks of 63 bits, samples of 32 blocks
    uint64_t cls_img_wpl;       // class words of a level in an image: 192 bits per sample (whole samples: select_in reads a sample's six words)
    uint64_t cls_wpl;           // as stored: + two pad words (even: 8-byte loads)
    uint64_t nrank_n, dstab_n;  // entries of d_nrank (every node start of every level + the level's total) and d_dstab (two per entry)
    uint32_t level_tiles;       // workgroups of k_wt_level: tiles of 256 stored words
    uint64_t state_per_level;   // scan-state words of a level's pass: one per tile + the ticket counter
    // element counts of the object's device arrays (0: the coding does not have the array); d_offs: wt_off_base(...)[L]
    uint64_t C_n, bits_n, rank_n, cls_n, samp_n /* d_ptr and d_rs each */, binom_n;
    // words of an image
    uint64_t img_bits_n, img_cls_n;
};
constexpr uint64_t WT_BINOM_WORDS = 64 * 64 + 8;  // C(n, k), n, k < 64; behind them the 64 offset widths as bytes
inline WtGeom wt_geom(uint64_t nlist, uint64_t ntotal, int wt_type) {
    WtGeom g{};
    const bool rrr = wt_type == 1;
    g.wt_type = wt_type;
    g.L = wt_levels(nlist);
    g.ntotal = ntotal;
    g.W = wt_words(ntotal);
    g.words_per_level = g.W + 1;
    g.blocks_per_level = (g.words_per_level + dev::BLK_WORDS - 1) / dev::BLK_WORDS;
    g.nblk = (ntotal + dev::RRR_B - 1) / dev::RRR_B;
    g.nsamp = (g.nblk + dev::RRR_K - 1) / dev::RRR_K;
    g.cls_img_wpl = 6 * g.nsamp;
    g.cls_wpl = g.cls_img_wpl + 2;
    g.nrank_n = dev::wt_nrank_base(g.L) + 1;
    g.dstab_n = 2 * g.nrank_n;
    g.level_tiles = (uint32_t)((g.words_per_level + VIDC_WT_EPT * 4 - 1) / (VIDC_WT_EPT * 4));
    g.state_per_level = (uint64_t)g.level_tiles + 1;
    g.C_n = nlist + 1;
    g.bits_n = rrr ? 0 : g.L * g.words_per_level;
    g.rank_n = rrr ? 0 : g.L * (g.blocks_per_level + 1);
    g.cls_n = rrr ? g.L * g.cls_wpl : 0;
    g.samp_n = rrr ? g.L * (g.nsamp + 1) : 0;
    g.binom_n = rrr ? WT_BINOM_WORDS : 0;
    g.img_bits_n = rrr ? 0 : g.L * g.W;
    g.img_cls_n = rrr ? g.L * g.cls_img_wpl : 0;
    return g;
}

// ---- offset streams (wt_type 1), sizes.  off_bits: [L] bits of every level's offset stream (ignored for wt_type 0, may be NULL)
// first word of every level's stream in d_offs, [L + 1]: exact-size streams level after level, + one pad word each (two-word reads)
inline std::vector<uint64_t> wt_off_base(const WtGeom &g, const uint64_t *off_bits) {
    std::vector<uint64_t> base(g.L + 1, 0);
    for (uint32_t l = 0; l < g.L; l++) base[l + 1] = base[l] + wt_words(off_bits[l]) + 1;
    return base;
}
struct WtImageWords { uint64_t n_bits, n_cls, n_offs; };
inline WtImageWords wt_image_words(const WtGeom &g, const uint64_t *off_bits) {
    WtImageWords iw{g.img_bits_n, g.img_cls_n, 0};
    if (g.wt_type == 1)
        for (uint32_t l = 0; l < g.L; l++) iw.n_offs += wt_words(off_bits[l]);  // (without the pad words)
    return iw;
}
// size accounting = what the object holds: plain bits + rank directory, or the RRR arrays (packed classes, offset streams,
// samples); + the symbol start table
inline uint64_t wt_size_bytes(const WtGeom &g, uint64_t nlist, const uint64_t *off_bits) {
    if (g.wt_type == 0) return (uint64_t)g.L * (g.W * 8 + (g.blocks_per_level + 1) * 4) + (nlist + 1) * 8;
    uint64_t ob = 0;
    for (uint32_t l = 0; l < g.L; l++) ob += off_bits[l];
    return (ob + 7) / 8 + (uint64_t)g.L * ((6 * g.nblk + 7) / 8) + (uint64_t)g.L * (g.nsamp + 1) * 8 + (nlist + 1) * 8;
}

// ---- build
struct WtBuildPolicy {
    bool direct_scatter = false;  // VIDC_WT_SCATTER (per call): the direct scatter at every size
    int num_cu = 0;
};
struct WtBuildPlan {
    // list_nos[id]: partition + place (two streaming passes) for the sizes it is built for, the direct scatter otherwise
    bool part2 = false;
    uint32_t nbuckets = 0;                      // part2: workgroups of k_wt_part_place
    uint32_t scatter_grid = 0, check_grid = 0;  // direct: k_wt_scatter_syms (launched when there are ids), k_wt_check_syms
    uint32_t nr_grid = 0;                       // k_wt_node_ranks_from_C
    uint32_t rrr_block_grid = 0, rrr_sample_grid = 0;  // wt_type 1: k_rrr_classes / k_rrr_offsets, k_rrr_samples
    // scratch, in elements
    uint64_t syms_n = 0;   // each of the two symbol arrays (u32)
    uint64_t part_n = 0;   // part2: per-workgroup histograms, bucket totals, bucket starts (u32)
    uint64_t state_n = 0;  // scan states of every level's pass (u64)
    // wt_type 1: one level of plain bits (u64) and its rank directory (u32), offset widths (u32) and bit positions (u64) of the
    // level's blocks, and per level the worst case of its offset stream, 61 bits per block (u64; the object keeps the exact size)
    uint64_t lvl_bits_n = 0, lvl_rank_n = 0, width_n = 0, bitpos_n = 0, offs_tmp_per_level = 0, offs_tmp_n = 0;
};
inline uint32_t wt_nr_grid(const WtGeom &g) { return g.L * VIDC_WT_NR_G; }
inline WtBuildPlan wt_build_plan(const WtGeom &g, uint64_t nlist, const WtBuildPolicy &p) {
    WtBuildPlan pl;
    const uint64_t nt = g.ntotal, cap = (uint64_t)p.num_cu * 32;
    pl.part2 = nt >= VIDC_WTP_MIN_IDS && nt <= VIDC_WTP_MAX_IDS && nlist <= VIDC_WTP_MAX_LISTS && !p.direct_scatter;
    if (pl.part2) {
        pl.nbuckets = (uint32_t)((nt + VIDC_WTP_BUCKET - 1) >> VIDC_WTP_BSH);
        pl.part_n = (uint64_t)VIDC_WTP_NBLK * VIDC_WTP_MAXB + 2 * VIDC_WTP_MAXB + 8;
    } else {
        pl.scatter_grid = (uint32_t)std::min<uint64_t>((nt + 4095) / 4096, cap);
        pl.check_grid = (uint32_t)std::min<uint64_t>((nt + 255) / 256 + 1, cap);
    }
    pl.nr_grid = wt_nr_grid(g);
    pl.syms_n = nt ? nt : 1;
    pl.state_n = (uint64_t)g.L * g.state_per_level;
    if (g.wt_type == 1) {
        pl.rrr_block_grid = (uint32_t)std::min<uint64_t>((g.nblk + 255) / 256 + 1, cap);
        pl.rrr_sample_grid = (uint32_t)std::min<uint64_t>(g.nsamp / 256 + 1, 4096);
        pl.lvl_bits_n = g.words_per_level;
        pl.lvl_rank_n = g.blocks_per_level + 1;
        pl.width_n = pl.bitpos_n = g.nblk + 1;
        pl.offs_tmp_per_level = g.words_per_level + 1;
        pl.offs_tmp_n = (uint64_t)g.L * pl.offs_tmp_per_level;
    }
    return pl;
}

// ---- bulk decode (vidc_wt_decode_all, ntotal > 0): L stable partitions over tiles of 256 * VIDC_WTD_EPT positions
struct WtDecodePlan {
    uint32_t tile_grid = 0;
    uint32_t expand_grid = 0, rankdir_grid = 0;  // wt_type 1: k_rrr_expand, k_rrr_rankdir
    uint32_t item_arrays = 0;                    // ping-pong (id, symbol prefix) arrays: none for one level, one for two
    uint64_t items_n = 0;                        // elements of each
    uint64_t lvl_bits_n = 0, lvl_rank_n = 0;     // wt_type 1: one level as plain bits (u64) + rank directory (u32)
};
inline WtDecodePlan wt_decode_plan(const WtGeom &g, int num_cu) {
    WtDecodePlan pl;
    pl.tile_grid = (uint32_t)((g.ntotal + 256u * VIDC_WTD_EPT - 1) / (256u * VIDC_WTD_EPT));
    pl.item_arrays = g.L > 2 ? 2u : g.L - 1u;
    pl.items_n = g.ntotal;
    if (g.wt_type == 1) {
        pl.expand_grid = (uint32_t)std::min<uint64_t>((g.nblk + 255) / 256, (uint64_t)num_cu * 32);
        pl.rankdir_grid = (uint32_t)std::min<uint64_t>((g.blocks_per_level + 256) / 256, 1024);
        pl.lvl_bits_n = g.words_per_level;
        pl.lvl_rank_n = g.blocks_per_level + 1;
    }
    return pl;
}

// ---- import: the passes that rebuild the rank directory (wt_type 0) or the samples (wt_type 1) and check the image on the device.
// Grids are the x dimension; y is the level wherever a pass takes every level in one launch.
struct WtImportPlan {
    uint32_t node_grid = 0;    // k_wt_imp_check_nodes
    uint32_t ones_grid = 0;    // wt_type 0: k_wt_imp_block_ones
    uint32_t prefix_grid = 0;  // k_wt_imp_level_prefix over the rank blocks / the samples
    uint32_t sums_grid = 0;    // wt_type 1: k_wt_imp_sample_sums (launched when there are samples)
    uint32_t blocks_grid = 0;  // wt_type 1: k_wt_imp_check_blocks (launched when there are blocks)
    uint64_t per_level = 0;    // rank blocks / samples of a level: what the scans run over, the levels back to back
    uint64_t sum_n = 0;        // scratch: sums to scan (u32; two arrays for wt_type 1)
    uint64_t scan_n = 0;       // scratch: their prefixes (u64; two arrays for wt_type 1)
    uint64_t err_n = 0;        // scratch (u64): the error word, the levels' width totals
};
inline WtImportPlan wt_import_plan(const WtGeom &g, int num_cu) {
    WtImportPlan pl;
    pl.node_grid = (uint32_t)std::min<uint64_t>(((1ull << (g.L - 1)) + 1 + 255) / 256, 4096);
    pl.per_level = g.wt_type == 1 ? g.nsamp : g.blocks_per_level;
    const uint64_t n = (uint64_t)g.L * pl.per_level;
    pl.prefix_grid = (uint32_t)std::min<uint64_t>((pl.per_level + 256) / 256, 1024);
    if (g.wt_type == 1) {
        pl.sums_grid = (uint32_t)((g.nsamp + 255) / 256);
        pl.blocks_grid = (uint32_t)std::min<uint64_t>((g.nblk + 255) / 256, (uint64_t)num_cu * 8);
        pl.sum_n = n ? n : 1;
    } else {
        pl.ones_grid = (uint32_t)((g.blocks_per_level * 8 + 255) / 256);
        pl.sum_n = n;
    }
    pl.scan_n = n + 1;
    pl.err_n = 1 + (uint64_t)g.L;
    return pl;
}

// ---- the host checks of an image (vidc_wt_import, before anything reaches the device): the shape, the offsets, the sizes the
// geometry demands of the arrays, and every bit of the arrays that lies behind what the geometry uses
enum WtImageKind {
    WT_IMG_OK,
    WT_IMG_TYPE,           // a = wt_type
    WT_IMG_NLIST,
    WT_IMG_OFFSETS_START,  // offsets[0] != 0
    WT_IMG_OFFSETS_ORDER,  // a = the list at which the offsets decrease
    WT_IMG_NTOTAL,
    WT_IMG_N_BITS,         // a = n_bits, b = the words the offsets need (or bits is NULL)
    WT_IMG_PLAIN_EXTRA,    // wt_type 0 with n_cls or n_offs
    WT_IMG_BITS_STRAY,     // level: a bit behind position ntotal in the level's last word
    WT_IMG_RRR_EXTRA,      // wt_type 1 with n_bits
    WT_IMG_N_CLS,          // a = n_cls, b = the words the offsets need (or cls is NULL)
    WT_IMG_OFF_BITS_NULL,
    WT_IMG_OFF_BITS_MAX,   // level, a = off_bits[level] > 61 bits per block (the widest offset has 61 bits)
    WT_IMG_N_OFFS,         // a = n_offs, b = the words off_bits needs (or offs is NULL)
    WT_IMG_CLS_STRAY,      // level: a class field behind the last block
    WT_IMG_OFFS_STRAY      // level: an offset bit behind off_bits[level]
};
struct WtImageVerdict {
    WtImageKind kind;
    uint32_t level;
    uint64_t a, b;
};
// offsets: not NULL, nlist + 1 entries once nlist is accepted
inline WtImageVerdict wt_image_check(uint64_t nlist, const uint64_t *offsets, int wt_type, const uint64_t *bits, uint64_t n_bits,
                                     const uint32_t *cls, uint64_t n_cls, const uint64_t *offs, uint64_t n_offs, const uint64_t *off_bits) {
    const WtShape shape = wt_shape_check(nlist, 0, wt_type);
    if (shape == WT_SHAPE_TYPE) return {WT_IMG_TYPE, 0, (uint64_t)(int64_t)wt_type, 0};
    if (shape == WT_SHAPE_NLIST) return {WT_IMG_NLIST, 0, nlist, 0};
    if (offsets[0] != 0) return {WT_IMG_OFFSETS_START, 0, offsets[0], 0};
    for (uint64_t l = 0; l < nlist; l++)
        if (offsets[l + 1] < offsets[l]) return {WT_IMG_OFFSETS_ORDER, 0, l, 0};
    const uint64_t nt = offsets[nlist];
    if (!wt_ntotal_ok(nt)) return {WT_IMG_NTOTAL, 0, nt, 0};
    const WtGeom g = wt_geom(nlist, nt, wt_type);
    if (wt_type == 0) {
        if (n_bits != g.img_bits_n || (n_bits && !bits)) return {WT_IMG_N_BITS, 0, n_bits, g.img_bits_n};
        if (n_cls || n_offs) return {WT_IMG_PLAIN_EXTRA, 0, n_cls, n_offs};
        if (nt & 63u)
            for (uint32_t l = 0; l < g.L; l++)
                if (bits[(uint64_t)l * g.W + g.W - 1] >> (nt & 63u)) return {WT_IMG_BITS_STRAY, l, 0, 0};
        return {WT_IMG_OK, 0, 0, 0};
    }
    if (n_bits) return {WT_IMG_RRR_EXTRA, 0, n_bits, 0};
    if (n_cls != g.img_cls_n || (n_cls && !cls)) return {WT_IMG_N_CLS, 0, n_cls, g.img_cls_n};
    if (!off_bits) return {WT_IMG_OFF_BITS_NULL, 0, 0, 0};
    for (uint32_t l = 0; l < g.L; l++)
        if (off_bits[l] > 61 * g.nblk) return {WT_IMG_OFF_BITS_MAX, l, off_bits[l], 61 * g.nblk};
    const uint64_t need = wt_image_words(g, off_bits).n_offs;
    if (n_offs != need || (n_offs && !offs)) return {WT_IMG_N_OFFS, 0, n_offs, need};
    uint64_t at = 0;
    for (uint32_t l = 0; l < g.L; l++) {
        for (uint64_t b = g.nblk; b < g.nsamp * dev::RRR_K; b++) {  // class fields behind the last block (fewer than 32)
            const uint64_t bp = 6 * b;
            uint64_t f = (uint64_t)cls[(uint64_t)l * g.cls_img_wpl + (bp >> 5)] >> (bp & 31);
            if ((bp & 31) > 26) f |= (uint64_t)cls[(uint64_t)l * g.cls_img_wpl + (bp >> 5) + 1] << (32 - (bp & 31));
            if (f & 63u) return {WT_IMG_CLS_STRAY, l, b, 0};
        }
        const uint64_t ow = wt_words(off_bits[l]);
        if ((off_bits[l] & 63u) && (offs[at + ow - 1] >> (off_bits[l] & 63u))) return {WT_IMG_OFFS_STRAY, l, 0, 0};
        at += ow;
    }
    return {WT_IMG_OK, 0, 0, 0};
}

}  // namespace vidc
