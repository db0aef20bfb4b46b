// graph_search_views.h -- what graph_search.hip reads of the two graph-row objects, whose structs stay private to their translation
// units (packed.hip, ef.hip).  Not part of the C-ABI.  The pointers are the objects' own device arrays: nothing is copied or built.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct vidc_compact;
struct vidc_ef;

namespace vidc {

struct CompactRowsView {
    const uint8_t *data;  // N * stride row bytes + 8 padding bytes
    uint64_t N;
    uint32_t K, bits, stride;
};
void compact_rows_view(const ::vidc_compact *c, CompactRowsView *out);

struct EfRowsView {
    bool rows;    // built from graph rows
    bool arena;   // ... of at most 64 edges: the fixed-stride arena exists
    const uint64_t *arena_words;  // row i: words [i * (LW + HW), (i + 1) * (LW + HW)), LW low words in front of HW high words
    const uint2 *meta;            // {universe, n | l << 8} per row
    uint64_t N;
    uint32_t K, LW, HW;
};
void ef_rows_view(const ::vidc_ef *e, EfRowsView *out);

}  // namespace vidc
