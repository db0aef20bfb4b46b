/*
 * vidc.h -- C-ABI of the MI355X-native vector-ID codec library (libvidc.so).
 *
 * Drop-in boundary for the per-inverted-list ID codecs of
 * facebookresearch/vector_db_id_compression.  Plain pointers and sizes only; no Faiss,
 * torch or C++ types cross this boundary.  Every entry point names the reference
 * interface it replaces (file:line under /root/reference).
 *
 * Data model: a set of lists is a CSR pair  offsets[nlist+1] (host, uint64) + ids[ntotal].  The *_encode_dev /
 * vidc_wt_build_dev entry points take the offsets as a DEVICE array instead (lists built on the GPU).
 * IDs are faiss::idx_t viewed as uint64 (custom_invlists_impl.cpp:79,159,217,248) or int32
 * graph rows (altid_impl.cpp:26-37).  "dev" pointers are HIP device pointers valid on the
 * context's device; everything else is host memory.  Out-buffers are caller-allocated.
 *
 * Error convention: every call returns VIDC_OK (0) or a negative vidc_status;
 * vidc_last_error() returns a thread-local message (replaces FAISS_THROW_IF_NOT /
 * FaissException, custom_invlists_impl.cpp:87,420-422 and custom_invlists.swig:38-57).
 * There is NO CPU fallback: without a HIP device vidc_ctx_create fails with VIDC_ERR_NO_DEVICE.
 *
 * Residency: compressed objects live on the device, including their per-list metadata (offsets, word counts,
 * precisions, ...).  Sizes come back as scalars; the *_list_info / *_export_* calls copy the per-list arrays to the
 * host on first use.  Device memory of objects and scratch comes from a block cache shared by the context and the
 * objects created through it (steady-state calls neither hipMalloc nor hipFree); objects may be destroyed before
 * or after their context.
 *
 * Environment (test hooks, read per call): VIDC_NO_LANE=1 / VIDC_FORCE_LANE=1 never / always use the
 * lane-per-list ROC kernels (default: only for calls with thousands of short lists), VIDC_FORCE_GENERAL=1 routes
 * every list through the general wave-per-list kernels, VIDC_HOST_THREADS=n caps the host threads used to plan calls
 * with >= 131072 lists (default 8), VIDC_TRACE=1 prints host-side phase times.  Read when a context is created:
 * VIDC_WIDE_STREAMS=1 (behave as if GPU_MAX_HW_QUEUES >= 8), VIDC_NUM_CU=n (size grids as if the device had n < its own
 * count of compute units, see vidc_ctx_num_cu), VIDC_POOL_POISON=1.  The bit streams do not depend on any of them.
 */
#ifndef VIDC_H
#define VIDC_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIDC_VERSION 100

typedef enum {
    VIDC_OK = 0,
    VIDC_ERR_INVALID = -1,     /* bad argument */
    VIDC_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime error at init */
    VIDC_ERR_HIP = -3,         /* HIP runtime error (message has hipGetErrorString) */
    VIDC_ERR_DOMAIN = -4,      /* input outside the codec's domain (id >= 2^31, id >= ntotal, list too long) */
    VIDC_ERR_OVERFLOW = -5,    /* internal arena / mt19937 table exhausted */
    VIDC_ERR_UNSUPPORTED = -6
} vidc_status;

const char *vidc_last_error(void);
int vidc_version(void);

/* ------------------------------------------------------------------ context */
typedef struct vidc_ctx vidc_ctx;
/* device < 0 : current HIP device.  Creates the context's own stream. */
int vidc_ctx_create(int device, vidc_ctx **out);
void vidc_ctx_destroy(vidc_ctx *ctx);
/* Run on a caller-owned hipStream_t (e.g. torch's current stream).  NULL is the legacy default stream (what
 * torch uses unless told otherwise); vidc_ctx_reset_stream goes back to the context's own stream. */
int vidc_ctx_set_stream(vidc_ctx *ctx, void *hip_stream);
int vidc_ctx_reset_stream(vidc_ctx *ctx);
int vidc_ctx_synchronize(vidc_ctx *ctx);
/* A context caches the device and pinned-host blocks its calls used (steady-state encode / decode calls neither
 * allocate nor free; a 10^9-id decode leaves several GB of scratch behind).  vidc_ctx_trim synchronises the
 * context's stream and releases every cached block that is not in use; *freed_bytes (optional) = device + pinned
 * bytes returned to the driver.  Blocks held by live objects are untouched.  The process-wide cache of emptied host arrays
 * (kept so that the next 10^6-list encode does not page-fault ~50 MB in again; bounded at 256 MB per element type) is
 * released as well. */
int vidc_ctx_trim(vidc_ctx *ctx, uint64_t *freed_bytes);
/* Test aid: fill every device block the context's cache hands out with 0xFF first (also: VIDC_POOL_POISON=1 in the environment when the
 * context is created).  Streams must not depend on what a block held before. */
int vidc_ctx_debug_pool_poison(vidc_ctx *ctx, int on);
/* Streams the kernel classes of one large ROC call are spread over: 8 when the PROCESS was started with the ROCm runtime
 * variable GPU_MAX_HW_QUEUES >= 8 (HIP multiplexes a process's streams onto that many hardware queues, default 4, and reads
 * the variable when it initialises: export it before the process starts -- for a Faiss-hosted process in the environment of
 * the Python / C++ program that loads Faiss, not after `import faiss`), otherwise 4.  The published S2 numbers are the 8-stream
 * mode; the 4-stream mode is ~10 % slower on calls of ~10^6 lists and identical on small calls.  Returns 0 for NULL. */
int vidc_ctx_class_streams(const vidc_ctx *ctx);
/* Compute units the context sizes its grids by: the device's multiProcessorCount, unless VIDC_NUM_CU=n was in the environment when
 * the context was created (test hook).  The hook can only LOWER the count: it applies for 1 <= n < the device's own count and is
 * ignored otherwise (0, not a number, at or above the device's count), so a grid never exceeds what the device holds -- the graph
 * compaction kernel relies on every wavefront of its launch being resident.  With a small n the grid-stride loops of the kernels take
 * several trips at sizes where they would otherwise take one; the output does not depend on it.  Returns 0 for NULL. */
uint32_t vidc_ctx_num_cu(const vidc_ctx *ctx);
/* Device memory helpers for hosts without their own allocator (Python uses torch tensors instead). */
int vidc_dev_alloc(vidc_ctx *ctx, size_t bytes, void **dev_ptr);
int vidc_dev_free(vidc_ctx *ctx, void *dev_ptr);
int vidc_copy_h2d(vidc_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
int vidc_copy_d2h(vidc_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);
/* Bytes of id payload this context has copied device -> host so far (vidc_copy_d2h, the *_get selects, *_decode_gather):
 * what a deferred search costs on PCIe -- 8 bytes per result through *_decode_gather, whole lists through
 * *_decode_lists + vidc_copy_d2h.  Metadata read-backs (sizes, status words, list_info) are not counted. */
uint64_t vidc_ctx_d2h_bytes(const vidc_ctx *ctx);

/* ------------------------------------------------------- ROC (bits-back ANS) */
/* Replaces: ANSState (codec.h:13-45), compress/decompress (codec.cpp:123-152),
 * CompressedIDInvertedListsFenwickTree ctor/get_ids (custom_invlists_impl.cpp:133-223),
 * ROCNSGGraph ctor/get_neighbors (altid_impl.cpp:103-165).
 * Bitstreams (head + 32-bit stack words) are bit-identical to codec.cpp. */
typedef struct vidc_roc vidc_roc;

/* precision_mode for vidc_roc_encode */
#define VIDC_PREC_REFERENCE (-1) /* ceil(log2((int)max_id)), custom_invlists_impl.cpp:163-164 (pow-2 quirk kept) */
#define VIDC_PREC_EXACT (-2)     /* bit_width(max_id): lossless for pow-2 max ids (NOT reference-identical) */
/* precision_mode >= 0 : fixed precision for every list (compress(n,data,state,precision), codec.cpp:123) */

#define VIDC_ROC_WANT_PERM 1u /* keep the sampling permutation (code re-ordering, custom_invlists_impl.cpp:188-193) */

/* Encode every list.  d_ids: device uint64[ntotal].  offsets: host uint64[nlist+1].
 * Lists may be unsorted and may be empty.  Domain: ids < 2^31 (reference `int max_id`), n <= VIDC_ROC_MAX_LIST. */
#define VIDC_ROC_MAX_LIST 262144u
int vidc_roc_encode(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, const uint64_t *d_ids,
                    int precision_mode, uint32_t flags, vidc_roc **out);
/* device offsets: see vidc_packed_encode_dev.  The call copies d_offsets to the host once and runs vidc_roc_encode's planner
 * on that copy: an O(nlist) D2H copy and host pass (ROC is bound by its ANS chains, not by this copy). */
int vidc_roc_encode_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal,
                        const uint64_t *d_ids, int precision_mode, uint32_t flags, vidc_roc **out);
/* Graph rows: d_rows device int32[N*K], -1 terminated rows (altid_impl.cpp:110-117). */
int vidc_roc_encode_rows(vidc_ctx *ctx, uint64_t N, uint32_t K, const int32_t *d_rows, int precision_mode,
                         uint32_t flags, vidc_roc **out);
void vidc_roc_destroy(vidc_roc *r);

uint64_t vidc_roc_nlist(const vidc_roc *r);
uint64_t vidc_roc_ntotal(const vidc_roc *r);
/* sum over non-empty lists of 8 + 4*nwords  (ANSState::size(), codec.h:42-44; :196-206) */
uint64_t vidc_roc_compressed_bytes(const vidc_roc *r);
uint64_t vidc_roc_total_words(const vidc_roc *r);
/* host copies of per-list metadata (arrays of nlist): any pointer may be NULL.  The metadata lives on the device;
 * the first call copies it to the host (blocking). */
int vidc_roc_list_info(const vidc_roc *r, uint32_t *sizes, uint32_t *precisions, uint64_t *heads,
                       uint32_t *nwords, uint32_t *mt_draws);
/* stack words of one list, push order (parity export).  cap in words. */
int vidc_roc_export_words(vidc_ctx *ctx, const vidc_roc *r, uint64_t list_no, uint32_t *words, size_t cap);
/* the whole compact stream (lists back to back, vidc_roc_total_words() words) in one copy */
int vidc_roc_export_all_words(vidc_ctx *ctx, const vidc_roc *r, uint32_t *words, size_t cap);
/* sampling permutation for all lists: perm[offsets[l]+i] = input position of the i-th sampled id */
int vidc_roc_perm(vidc_ctx *ctx, const vidc_roc *r, uint32_t *perm_host);
const uint32_t *vidc_roc_perm_dev(const vidc_roc *r);
/* Build from exported streams (decode-only parity tests, on-disk reload).  All host arrays. */
int vidc_roc_import(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, const uint32_t *precisions,
                    const uint64_t *heads, const uint32_t *nwords, const uint32_t *mt_draws,
                    const uint32_t *words_concat, vidc_roc **out);
/* Regroup: a new IVF object made of whole lists of other objects, without encoding.  *out holds m lists on ctx; list j of it is list
 * list_no[j] of srcs[src_no[j]] (src_no, list_no: host arrays of m).  Size, precision, head, nwords, mt_draws and every stack word are
 * carried over bit for bit, so the list decodes exactly as it did in its source; no ANS step runs.  A list may be named more than
 * once; empty lists and lists with nwords == 0 are ordinary.  1 <= nsrc <= VIDC_SHARDS_MAX (declared with the sharded lists below: 8);
 * every source lives on ctx's device; an entry of srcs may be NULL as long as no src_no names it.  m == 0 is what vidc_roc_import makes
 * of nlist == 0: VIDC_OK and an object without lists (src_no and list_no may then be NULL).
 * flags: with VIDC_ROC_WANT_PERM *out carries the IDENTITY permutation in every list -- the convention of the append and the remove: a
 *   permutation of a derived object is over the positions of what the old lists decode to.  The sources need no permutation.
 * Like an imported object *out carries no planner hints (the decode planner mirrors the metadata on first use).
 * Status.  A NULL ctx / srcs / out, a NULL table with m > 0, nsrc outside its range, m >= 2^32 - 1, a src_no >= nsrc or one that names a
 *   NULL source (these before any source is looked into), a source on another device, a list_no >= its source's nlist:
 *   VIDC_ERR_INVALID before any device work.  A graph-row source: VIDC_ERR_UNSUPPORTED.  On any error *out == NULL.
 * What runs, all on the context's stream: the (src_no, list_no) table is uploaded (12 bytes per list); one kernel gathers the five
 *   per-list arrays from the sources, whose descriptors it takes by value; one scan turns sizes and word counts into the offsets and
 *   the word offsets; the word total is read back (8 bytes, the call's only read-back); a wavefront per 1024-word chunk copies the
 *   streams (16-byte accesses where source and destination agree mod 16, behind a head of at most three words -- the copy loop of
 *   the append's and the remove's splice).  No atomic decides a position and nothing spins.  The call synchronises;
 *   vidc_ctx_last_kernel_ms covers these launches. */
int vidc_roc_regroup(vidc_ctx *ctx, int nsrc, const vidc_roc *const *srcs, uint64_t m, const uint32_t *src_no /* host, m */,
                     const uint64_t *list_no /* host, m */, uint32_t flags, vidc_roc **out);

/* Decode every list into d_out (device uint64[ntotal], CSR order, each list in sampling order
 * = the order get_ids returns, codec.cpp:150). */
int vidc_roc_decode_all(vidc_ctx *ctx, const vidc_roc *r, uint64_t *d_out);
/* Decode m selected lists back to back into d_out; out_offsets (host, m+1) receives the packing. */
int vidc_roc_decode_lists(vidc_ctx *ctx, const vidc_roc *r, uint64_t m, const uint64_t *list_nos,
                          uint64_t *d_out, uint64_t *out_offsets);
/* The decode section of the deferred search in ONE call (custom_invlists_impl.cpp:508-525: `ids = get_ids(list_no)` per touched
 * list, then `labels[r] = ids[lo_offset(labels[r])]`): the m touched lists are decoded into device staging owned by the
 * context, the n_items requested ids are picked ON THE DEVICE (item i = list_nos[item_slot[i]][item_off[i]]) and only those
 * cross PCIe: 8 * n_items bytes into ids_out (host int64[n_items]).  Items outside their list -> VIDC_ERR_INVALID, reported before
 * anything is decoded.  list_nos should name every touched list ONCE (a repeated list is decoded and staged once per mention).
 * Same signature for the four containers (vidc_ef_decode_gather, vidc_packed_decode_gather, vidc_wt_decode_gather). */
int vidc_roc_decode_gather(vidc_ctx *ctx, const vidc_roc *r, uint64_t m, const uint64_t *list_nos, uint64_t n_items,
                           const uint64_t *item_slot, const uint64_t *item_off, int64_t *ids_out);
/* Graph flavour: d_out device int32[m*K]; rows padded with -1; counts (host, m, may be NULL) = num edges.
 * nodes == NULL selects nodes 0..m-1 (no index array is built or uploaded).  The first such call for every node of a graph of
 * 65 536 nodes or more also sorts the node numbers by edge count inside the object (4 bytes per node of device memory, 0.02 ms
 * at 10^6 nodes): rows of equal length then share a wavefront of the decoder; the output is the same rows in the same places. */
int vidc_roc_decode_rows(vidc_ctx *ctx, const vidc_roc *r, uint64_t m, const uint64_t *nodes, uint32_t K,
                         int32_t *d_out, uint32_t *counts);
/* End-state self check of the last decode_all: number of lists whose final ANS state is not the
 * initial one (head 2^31; SURVEY appendix A invariant).  Lossy reference cases (Q2/Q3) count here. */
uint64_t vidc_roc_last_decode_nonclean(const vidc_roc *r);
/* Work items of the object's last decode call that a bucket-row decoder handed back (a bucket of the list would have taken one
 * member more than its row holds) and that the call then decoded again, one after the other, on the general kernel: the output is
 * the same, the call pays a serial chain.  A list that the request names twice counts twice.  0 after a call without hand-backs. */
uint64_t vidc_roc_last_decode_handed_back(const vidc_roc *r);

/* -------------------------------------------------------------- packed bits */
/* Replaces CompressedIDInvertedListsPackedBits (custom_invlists_impl.cpp:64-118) and
 * CompactBitNSGGraph (altid_impl.cpp:20-51).  LSB-first, little-endian (reader :35-58). */
typedef struct vidc_packed vidc_packed;
int vidc_packed_bits_for(uint64_t ntotal); /* :68-70 */
int vidc_packed_encode(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, const uint64_t *d_ids, int bits,
                       vidc_packed **out);
/* Device offsets: d_offsets is a DEVICE uint64[nlist+1] on the context's device, read in order on the context's stream (the
 * caller orders its producer before the call, e.g. by running the context on torch's stream).  ntotal: the caller's id count
 * (= d_offsets[nlist], checked on the device, as are d_offsets[0] == 0 and monotone offsets: VIDC_ERR_INVALID naming the first
 * bad list).  The object keeps its own copy, so d_offsets may be freed or reused after the call returns.  Objects are the same
 * as the host-offsets calls produce, word for word.  Packed and wavelet tree: no O(nlist) host work or PCIe transfer, and no wait
 * beyond those of the host-offsets call.
 * Elias-Fano: the same; its chunk kernels read their count and form on the device (a list that is not ascending copies the
 * offsets to the host once, as the retry of the host path re-walks them; ids >= 2^32 take the host path's extra wait).  ROC: the length classes are planned on the host, so the offsets cross PCIe once (D2H). */
int vidc_packed_encode_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal,
                           const uint64_t *d_ids, int bits, vidc_packed **out);
/* host copy of the object's offsets[nlist+1] (objects from device offsets copy them from the device on first use) */
int vidc_packed_offsets(vidc_ctx *ctx, const vidc_packed *p, uint64_t *offsets);
void vidc_packed_destroy(vidc_packed *p);
uint64_t vidc_packed_compressed_bytes(const vidc_packed *p); /* sum ceil(ls*bits/8), :80,85 */
int vidc_packed_bits(const vidc_packed *p);
int vidc_packed_decode_all(vidc_ctx *ctx, const vidc_packed *p, uint64_t *d_out);
/* decode m selected lists back to back into d_out (get_ids per touched list, :96-105 / the loop :508-525);
 * out_offsets: host uint64[m + 1] */
int vidc_packed_decode_lists(vidc_ctx *ctx, const vidc_packed *p, uint64_t m, const uint64_t *list_nos, uint64_t *d_out,
                             uint64_t *out_offsets);
/* decode of the touched lists + device-side pick of the n_items requested ids (see vidc_roc_decode_gather) */
int vidc_packed_decode_gather(vidc_ctx *ctx, const vidc_packed *p, uint64_t m, const uint64_t *list_nos, uint64_t n_items,
                              const uint64_t *item_slot, const uint64_t *item_off, int64_t *ids_out);
/* m random accesses (get_single_id, :108-113): host arrays of list numbers / offsets -> host ids */
int vidc_packed_get(vidc_ctx *ctx, const vidc_packed *p, uint64_t m, const uint64_t *list_nos,
                    const uint64_t *offs, int64_t *ids_out);
/* byte image of one list (parity against the reference layout) */
int vidc_packed_export(vidc_ctx *ctx, const vidc_packed *p, uint64_t list_no, uint8_t *bytes, size_t cap);
/* Flat image {offsets, bits, words} for saving / shipping an object without re-encoding (the reference keeps compressed
 * lists in memory only): words = the device layout, every list starts on a 64-bit word and is followed by one padding
 * word. */
uint64_t vidc_packed_total_words(const vidc_packed *p);
int vidc_packed_export_all(vidc_ctx *ctx, const vidc_packed *p, uint64_t *words, size_t cap);
int vidc_packed_import(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, int bits, const uint64_t *words,
                       uint64_t nwords, vidc_packed **out);

/* CompactBitNSGGraph (altid_impl.cpp:20-51): N rows of K int32 (-1 terminated) -> N * stride bytes, sentinel N. */
typedef struct vidc_compact vidc_compact;
int vidc_compact_rows_encode(vidc_ctx *ctx, uint64_t N, uint32_t K, const int32_t *d_rows, vidc_compact **out);
void vidc_compact_destroy(vidc_compact *c);
uint32_t vidc_compact_bits(const vidc_compact *c);
uint32_t vidc_compact_stride(const vidc_compact *c);
uint64_t vidc_compact_size_in_bytes(const vidc_compact *c);
/* get_neighbors for m nodes: d_out device int32[m*K] (-1 padded), counts host uint32[m] (may be NULL);
 * nodes == NULL selects nodes 0..m-1 */
int vidc_compact_rows_decode(vidc_ctx *ctx, const vidc_compact *c, uint64_t m, const uint64_t *nodes, int32_t *d_out,
                             uint32_t *counts);
int vidc_compact_export_row(vidc_ctx *ctx, const vidc_compact *c, uint64_t node, uint8_t *bytes, size_t cap);
/* Flat image: the N * stride row bytes (row i at byte i * stride; field j of a row at bit j * bits, LSB first; the first -1 of a row
 * is the sentinel N, fields behind it are zero as the encoder writes them and are never decoded).  bits and stride follow from
 * (N, K) as in vidc_compact_rows_encode, with the same limits on K (VIDC_ERR_UNSUPPORTED); the import also returns
 * VIDC_ERR_UNSUPPORTED for an N that needs more than 32 bits per field (N >= 2^32: rows are int32, and the check and the decoders
 * read a field from two dwords); nbytes must equal N * stride.  The image is
 * untrusted input: a kernel checks that in every row each field up to and including the first sentinel is <= N (a decoded id >= N
 * would index past the caller's vectors), VIDC_ERR_INVALID otherwise, naming the first bad row.  All arrays are host memory. */
int vidc_compact_export_all(vidc_ctx *ctx, const vidc_compact *c, uint8_t *bytes, size_t cap); /* N * stride bytes */
int vidc_compact_import(vidc_ctx *ctx, uint64_t N, uint32_t K, const uint8_t *bytes, uint64_t nbytes, vidc_compact **out);

/* -------------------------------------------------------------- Elias-Fano */
/* Replaces CompressedIDInvertedListsEliasFano (custom_invlists_impl.cpp:229-339),
 * EliasFanoNSGGraph (altid_impl.cpp:53-101), succinct::elias_fano builder/select/enumerator
 * (elias_fano.hpp:22-57,141-145,210-261). */
typedef struct vidc_ef vidc_ef;
#define VIDC_EF_WANT_PERM 1u
int vidc_ef_encode(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, const uint64_t *d_ids, uint32_t flags,
                   vidc_ef **out);
/* device offsets: see vidc_packed_encode_dev */
int vidc_ef_encode_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal,
                       const uint64_t *d_ids, uint32_t flags, vidc_ef **out);
void vidc_ef_destroy(vidc_ef *e);
/* (sum low bits + sum high bits) / 8, custom_invlists_impl.cpp:272-282 */
uint64_t vidc_ef_compressed_bytes(const vidc_ef *e);
int vidc_ef_list_info(const vidc_ef *e, uint32_t *sizes, uint32_t *low_bits, uint64_t *universes);
int vidc_ef_decode_all(vidc_ctx *ctx, const vidc_ef *e, uint64_t *d_out); /* ascending per list, :305-308 */
int vidc_ef_get(vidc_ctx *ctx, const vidc_ef *e, uint64_t m, const uint64_t *list_nos, const uint64_t *offs,
                int64_t *ids_out); /* ef->select(offset), :314-318 */
int vidc_ef_perm(vidc_ctx *ctx, const vidc_ef *e, uint32_t *perm_host); /* sort permutation, :324-339 */
/* EliasFanoNSGGraph (altid_impl.cpp:53-101): rows are counted (-1 terminated), sorted and coded per node. */
int vidc_ef_encode_rows(vidc_ctx *ctx, uint64_t N, uint32_t K, const int32_t *d_rows, vidc_ef **out);
/* get_neighbors for m nodes: d_out device int32[m*K] ascending, -1 padded; counts host uint32[m] (may be NULL);
 * nodes == NULL selects nodes 0..m-1.
 * Output contract, the same for host nodes, nodes == NULL and device nodes (vidc_ef_decode_rows_dev): any K >= the widest requested
 * row is served, also K above the K the object was built with and K > 64; after the call EVERY one of the m * K elements is defined
 * -- a row's ids, then -1 up to column K - 1 -- whatever d_out held before, and no byte outside d_out[0 .. m*K) is written.  d_out
 * needs 4-byte alignment only. */
int vidc_ef_decode_rows(vidc_ctx *ctx, const vidc_ef *e, uint64_t m, const uint64_t *nodes, uint32_t K, int32_t *d_out,
                        uint32_t *counts);
/* decode m selected lists back to back (get_ids per touched list, custom_invlists_impl.cpp:508-525) */
int vidc_ef_decode_lists(vidc_ctx *ctx, const vidc_ef *e, uint64_t m, const uint64_t *list_nos, uint64_t *d_out,
                         uint64_t *out_offsets);
/* decode of the touched lists + device-side pick of the n_items requested ids (see vidc_roc_decode_gather) */
int vidc_ef_decode_gather(vidc_ctx *ctx, const vidc_ef *e, uint64_t m, const uint64_t *list_nos, uint64_t n_items,
                          const uint64_t *item_slot, const uint64_t *item_off, int64_t *ids_out);
/* word images of one list's low / high streams (64-bit words, LSB-first) */
int vidc_ef_export(vidc_ctx *ctx, const vidc_ef *e, uint64_t list_no, uint64_t *low, size_t low_cap,
                   uint64_t *high, size_t high_cap, uint64_t *low_nbits, uint64_t *high_nbits);
/* Flat image {offsets, l[], universe[], low[], high[]}: stream offsets follow from (count, l, universe) per list
 * (elias_fano.hpp:28-29); the select directory is rebuilt from the high stream on import. */
int vidc_ef_stream_words(const vidc_ef *e, uint64_t *low_words, uint64_t *high_words);
int vidc_ef_export_all(vidc_ctx *ctx, const vidc_ef *e, uint64_t *low, size_t low_cap, uint64_t *high, size_t high_cap);
int vidc_ef_import(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, const uint32_t *lbits,
                   const uint64_t *universe, const uint64_t *low, uint64_t n_low, const uint64_t *high, uint64_t n_high,
                   vidc_ef **out);

/* ------------------------------------------------------------ wavelet tree */
/* Replaces CompressedIDInvertedListsWaveletTree (custom_invlists_impl.cpp:346-397): one tree over the
 * sequence list_nos[id]; get_single_id(list, offset) = select(offset + 1, list) (:377-379).
 * Requires what the reference asserts (:359-360): ids ascending inside every list and ids a permutation
 * of 0..ntotal-1.  wt_type 0 = plain bitvectors, 1 = sizes reported for rrr_vector<63>-coded levels
 * (custom_invlists_impl.h:104-113); sdsl itself is absent, so sizes follow the documented layouts. */
typedef struct vidc_wt vidc_wt;
int vidc_wt_build(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, const uint64_t *d_ids, int wt_type,
                  vidc_wt **out);
/* device offsets: see vidc_packed_encode_dev */
int vidc_wt_build_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal,
                      const uint64_t *d_ids, int wt_type, vidc_wt **out);
int vidc_wt_offsets(vidc_ctx *ctx, const vidc_wt *w, uint64_t *offsets); /* see vidc_packed_offsets */
void vidc_wt_destroy(vidc_wt *w);
uint64_t vidc_wt_size_in_bytes(const vidc_wt *w);
uint32_t vidc_wt_levels(const vidc_wt *w);
int vidc_wt_select(vidc_ctx *ctx, const vidc_wt *w, uint64_t m, const uint64_t *list_nos, const uint64_t *offs,
                   int64_t *ids_out);
int vidc_wt_decode_all(vidc_ctx *ctx, const vidc_wt *w, uint64_t *d_out);
/* get_ids of m selected lists back to back (custom_invlists_impl.cpp:381-392 per list); out_offsets: host uint64[m + 1] */
int vidc_wt_decode_lists(vidc_ctx *ctx, const vidc_wt *w, uint64_t m, const uint64_t *list_nos, uint64_t *d_out,
                         uint64_t *out_offsets);
/* decode of the touched lists + device-side pick of the n_items requested ids (see vidc_roc_decode_gather) */
int vidc_wt_decode_gather(vidc_ctx *ctx, const vidc_wt *w, uint64_t m, const uint64_t *list_nos, uint64_t n_items,
                          const uint64_t *item_slot, const uint64_t *item_off, int64_t *ids_out);
/* Flat image for saving / shipping a tree without rebuilding it.  All arrays are host memory.
 * With L = vidc_wt_levels, nt = ntotal, W = ceil(nt / 64), nblk = ceil(nt / 63), nsamp = ceil(nblk / 32):
 *   offsets[nlist + 1]: the object's own offsets (vidc_wt_offsets).
 *   wt_type 0: bits = L * W words, level after level, without the object's internal pad word.  Bit i of level l is bit i & 63 of
 *     word l * W + (i >> 6); bits at positions >= nt are zero; n_cls = n_offs = 0.
 *   wt_type 1: n_bits = 0.  cls = L * 6 * nsamp 32-bit words, each level in whole samples: the class of block b of a level is the 6
 *     bits at bit 6 b of that level's words, LSB first -- the popcount of bits [63 b, 63 b + 63) of the level; class fields of blocks
 *     >= nblk are zero.  off_bits[l] = the sum over the level's blocks of ceil(log2 C(63, class)).  offs = the levels' offset streams
 *     back to back, ceil(off_bits[l] / 64) words each, unused top bits zero, without the object's pad words; a block's offset is its
 *     index among the 63-bit words with `class` ones in the combinatorial number system (the sum, over its ones in ascending order,
 *     i = 1 .. class, of C(position_i, i)).
 * The image does not carry the derived tables (they are not part of vidc_wt_size_in_bytes either): the 512-bit-block rank directory
 * (type 0), the (pointer, rank) samples (type 1) and the per-node rank tables (both) are rebuilt on the device by vidc_wt_import.
 * An image is untrusted input.  vidc_wt_import checks on the host: arguments and wt_type, 1 <= nlist < 2^32, offsets[0] == 0 and
 * monotone offsets, ntotal < 2^32 (VIDC_ERR_UNSUPPORTED, as vidc_wt_build), n_bits / n_cls / n_offs against what the geometry and
 * off_bits demand, zero pad bits / class fields / top bits; then on the device, before any position derived from the image is
 * followed: the per-level totals of the offset widths against off_bits, every RRR block (offset < C(63, class), class <= the bits the
 * block has, no one behind the level's end), and for every level l and node boundary p = 0 .. 2^l that the ones before position
 * offsets[min(p << (L - l), nlist)] equal what the offsets alone demand -- equal boundary counts mean every select and decode walk
 * finds the bit it looks for inside its node.  Any failure: VIDC_ERR_INVALID with a message naming the argument, or the first bad
 * (level, node); *out == NULL and the context stays usable.  An imported object is a built one to every other entry point. */
int vidc_wt_type(const vidc_wt *w); /* 0 / 1; -1 for NULL */
/* words of the three image arrays (any pointer may be NULL) */
int vidc_wt_image_words(const vidc_wt *w, uint64_t *n_bits, uint64_t *n_cls, uint64_t *n_offs);
int vidc_wt_export_all(vidc_ctx *ctx, const vidc_wt *w, uint64_t *bits, size_t bits_cap, uint32_t *cls, size_t cls_cap,
                       uint64_t *offs, size_t offs_cap, uint64_t *off_bits /* [levels], may be NULL for wt_type 0 */);
int vidc_wt_import(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets, int wt_type, const uint64_t *bits, uint64_t n_bits,
                   const uint32_t *cls, uint64_t n_cls, const uint64_t *offs, uint64_t n_offs, const uint64_t *off_bits,
                   vidc_wt **out);

/* ------------------------------------------- device-resident requests (labels, graph nodes) */
/* The decode section of a search that runs on the GPU: its labels (from a top-k) and its frontier (from an argmin) are device arrays
 * already, and these calls take them as such (custom_invlists_impl.cpp:508-525 as one call; get_neighbors, altid_impl.cpp).
 *
 * Labels.  A label is Faiss's lo_build(list_no, offset) = list_no << 32 | offset.  d_ids[i] = get_ids(list_no)[offset]: the id that
 *   vidc_*_decode_lists / vidc_*_decode_gather return for that pair, in the list's own order (sampling order for ROC, ascending for
 *   Elias-Fano and the wavelet tree, input order for packed bits).  A negative label (Faiss's "no result") gives -1 and is not counted.
 *   A label whose list is >= nlist, or whose offset is >= that list's size, is INVALID: it gives -1, and the call adds the number of
 *   such labels to *d_invalid (a device uint64 the caller zeroes; NULL: not counted).  d_ids == d_labels is allowed (in place).
 * Nodes.  A negative node gives a row of K times -1 and count 0, uncounted; a node >= N gives the same row and is counted in
 *   *d_invalid.  Rows and counts of the other nodes are those of the host-node calls (vidc_*_decode_rows, vidc_compact_rows_decode),
 *   which also fix which (object, K) pairs are accepted: K == 0 is rejected as there, a row with more than K edges fails as there.
 * Device pointers live on the context's device and are read and written in order on the context's stream.  d_counts (device uint32[m])
 *   and d_invalid may be NULL.  n == 0 / m == 0 returns VIDC_OK and launches nothing.  A NULL context or object, or a NULL array with
 *   n > 0 / m > 0, returns VIDC_ERR_INVALID before any device work.
 * Residency.  Packed bits, Elias-Fano and the wavelet tree (labels), compact rows and the rows of Elias-Fano graph objects with K >= the
 *   object's K (nodes): the call only ENQUEUES work -- no host work proportional to n / m, no PCIe transfer, no wait -- and does not
 *   update vidc_ctx_last_kernel_ms.  The first call on an object may build its lazy device tables as the host-array calls do (an
 *   Elias-Fano graph object gets its per-list streams, ef_ensure_csr, when it is translated); the first call with a larger request than
 *   the context has served before grows the context's request block in stream order (hipFreeAsync + hipMallocAsync on the
 *   context's stream: no host wait).
 *   ROC labels: the touched lists are marked and compacted on the device; their numbers (4 bytes per touched list, metadata: not
 *   counted in vidc_ctx_d2h_bytes) are read back once, the host plans their decode as vidc_roc_decode_lists does, the ids are picked
 *   on the device.  The call synchronises.
 *   ROC rows: on the lean lane path (graph object, K >= its K, a request of thousands of nodes, lane kernels not switched off) the nodes
 *   stay on the device (work list, counts and fix-up are kernels; the decode synchronises as vidc_roc_decode_rows does).  Other ROC
 *   requests, and Elias-Fano rows of list objects or of K < the object's K, copy the nodes to the host once (D2H) and run the host-node
 *   path (negative and invalid nodes ask it for the request's first valid node, whose row is then replaced by -1s), and wait.
 * The objects are read-only: concurrent calls on one object from different contexts behave as the host-array calls do. */
int vidc_packed_translate_labels_dev(vidc_ctx *ctx, const vidc_packed *p, uint64_t n, const int64_t *d_labels, int64_t *d_ids,
                                     uint64_t *d_invalid);
int vidc_ef_translate_labels_dev(vidc_ctx *ctx, const vidc_ef *e, uint64_t n, const int64_t *d_labels, int64_t *d_ids,
                                 uint64_t *d_invalid);
int vidc_wt_translate_labels_dev(vidc_ctx *ctx, const vidc_wt *w, uint64_t n, const int64_t *d_labels, int64_t *d_ids,
                                 uint64_t *d_invalid);
int vidc_roc_translate_labels_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t n, const int64_t *d_labels, int64_t *d_ids,
                                  uint64_t *d_invalid);
/* get_neighbors for a device-resident node array: d_nodes device int64[m], d_out device int32[m*K] (-1 padded: every column up to
 * K - 1 of every row is written at any accepted K, nothing outside d_out is; the output contract stated at vidc_ef_decode_rows). */
int vidc_compact_rows_decode_dev(vidc_ctx *ctx, const vidc_compact *c, uint64_t m, const int64_t *d_nodes, int32_t *d_out,
                                 uint32_t *d_counts, uint64_t *d_invalid);
int vidc_ef_decode_rows_dev(vidc_ctx *ctx, const vidc_ef *e, uint64_t m, const int64_t *d_nodes, uint32_t K, int32_t *d_out,
                            uint32_t *d_counts, uint64_t *d_invalid);
int vidc_roc_decode_rows_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t m, const int64_t *d_nodes, uint32_t K, int32_t *d_out,
                             uint32_t *d_counts, uint64_t *d_invalid);

/* ---------------------------------------------------- append (batches of ids, device-resident) */
/* Objects stay immutable: an append returns a NEW object in *out, the old one stays valid and unchanged, and either may be destroyed
 * first (the new object owns all of its memory).
 *
 * The batch.  Pair i is (d_list_nos[i], d_ids[i]): what a coarse quantizer on the GPU hands to `add`.  With old_l = list l of the old
 *   object in the object's own order (what vidc_*_decode_lists returns), the merged input of list l is
 *       M_l = old_l ++ [d_ids[i] for every i with d_list_nos[i] == l, in ascending i]
 *   -- the placement is stable: batch order inside a list is part of the contract.  A negative list number is skipped and not counted
 *   (Faiss's "not assigned"); a list number >= nlist is skipped and counted in *d_invalid (a device uint64 the caller zeroes; may be NULL).
 * The result is the object the existing encoder builds from the CSR form of M, word for word (streams, per-list metadata, sizes,
 *   compressed_bytes, and the permutation when the flag asks for it): vidc_packed_encode with `bits` (0 keeps the object's width; a
 *   larger width re-packs every list; an id that does not fit gives VIDC_ERR_DOMAIN), vidc_ef_encode with `flags`, vidc_wt_build with
 *   the object's wt_type (M must be what vidc_wt_build demands -- a permutation of 0 .. ntotal_new - 1, ascending inside each list --
 *   otherwise its status is returned), vidc_roc_encode with `precision_mode` and `flags` (the caller passes the mode the object was built
 *   with; the call cannot check it).  A permutation is over positions in M_l: j < |old_l| is the old entry at offset j, j >= |old_l| the
 *   (j - |old_l|)-th batch entry of that list.
 * ROC and duplicates.  The ROC stream of a list depends only on the multiset of its ids, and a decoded list of distinct ids re-encodes
 *   to the identity permutation; with duplicate ids inside one list the reference codec is lossy.  The result is defined through M as
 *   above whatever old_l decodes to; ids should be distinct inside every merged list (the IVF case).  A list the batch does not touch
 *   keeps its stream and gets the identity permutation: that is the from-scratch result whenever the list decodes to its own distinct
 *   ids (not for the reference's lossy cases -- duplicates, a power-of-two maximum under VIDC_PREC_REFERENCE, more than 65 536 ids).
 * Labels.  d_labels[i] (device int64[n_add], may be NULL) = list_no << 32 | offset at which batch entry i sits in the new object:
 *   vidc_*_translate_labels_dev on the new object gives back d_ids[i].  Skipped entries get -1.  The offset is |old_l| + the entry's
 *   rank in the batch (packed bits, wavelet tree), its position in the stable ascending order of M_l (Elias-Fano), its position in
 *   sampling order (ROC).
 * Arrays are device arrays on the context's device, read and written in order on the context's stream; n_add < 2^32 - 1.
 * Status.  NULL context, object or out, or a NULL array with n_add > 0: VIDC_ERR_INVALID before any device work.  A graph object (rows,
 *   Elias-Fano arena): VIDC_ERR_UNSUPPORTED.  A merged ROC list above VIDC_ROC_MAX_LIST, or an id >= 2^31: VIDC_ERR_DOMAIN.  On any
 *   error *out == NULL, the old object is untouched and the context stays usable.  n_add == 0, or a batch without a valid pair, returns
 *   an object equal to the old one.
 * Residency.  No id payload crosses PCIe (vidc_ctx_d2h_bytes does not move).  Packed bits, Elias-Fano and the wavelet tree are REBUILT:
 *   decode_all into scratch, the merge, the device-offsets encoder -- memory-rate kernels, one 8-byte read-back (the valid pair count),
 *   no O(nlist) array on the host.  ROC is SPLICED: only the lists the batch touches are decoded and re-encoded (their numbers and add
 *   counts are read back once, 8 bytes per touched list, and the host plans their classes as vidc_roc_translate_labels_dev does);
 *   every other list's stream is copied.  The calls synchronise. */
int vidc_packed_append_dev(vidc_ctx *ctx, const vidc_packed *p, uint64_t n_add, const int64_t *d_list_nos, const uint64_t *d_ids,
                           int bits, vidc_packed **out, int64_t *d_labels, uint64_t *d_invalid);
int vidc_ef_append_dev(vidc_ctx *ctx, const vidc_ef *e, uint64_t n_add, const int64_t *d_list_nos, const uint64_t *d_ids,
                       uint32_t flags, vidc_ef **out, int64_t *d_labels, uint64_t *d_invalid);
int vidc_wt_append_dev(vidc_ctx *ctx, const vidc_wt *w, uint64_t n_add, const int64_t *d_list_nos, const uint64_t *d_ids,
                       vidc_wt **out, int64_t *d_labels, uint64_t *d_invalid);
int vidc_roc_append_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t n_add, const int64_t *d_list_nos, const uint64_t *d_ids,
                        int precision_mode, uint32_t flags, vidc_roc **out, int64_t *d_labels, uint64_t *d_invalid);

/* ---------------------------------------------------- merge (two objects over the same lists, device-resident) */
/* Faiss's InvertedLists::merge_from(other, add_id): an index built in pieces, or sharded by id range, becomes one without leaving
 * the compressed form.  Objects stay immutable: a merge returns a NEW object in *out, `a` and `b` stay valid and unchanged, any of the
 * three may be destroyed first (the new object owns all of its memory), and a == b is allowed.
 *
 * The merged input.  With a_l and b_l = list l of each object in the object's own order (what vidc_*_decode_lists returns), the merged
 *   input of list l is
 *       M_l = a_l ++ [x + add_id for x in b_l]
 * The result is the object the existing encoder builds from the CSR form of M, word for word (streams, per-list metadata, sizes,
 *   compressed_bytes, and the permutation when the flag asks for it): vidc_packed_encode with `bits` (0 keeps a's width; a larger width
 *   re-packs every list; an id that does not fit gives VIDC_ERR_DOMAIN), vidc_ef_encode with `flags`, vidc_wt_build with a's wt_type (M
 *   must be what vidc_wt_build demands -- a permutation of 0 .. ntotal_new - 1, ascending inside each list; the usual add_id =
 *   ntotal(a) makes it so -- otherwise the build's status is returned), vidc_roc_encode with `precision_mode` and `flags` (the caller
 *   passes the mode the objects were built with; the call cannot check it).  A permutation is over positions in M_l: j < |a_l| is a's
 *   entry at offset j, j >= |a_l| is b's entry at offset j - |a_l|.
 * ROC.  A list with b_l empty keeps a's stream; a list with a_l empty and add_id == 0 keeps b's stream; both get the identity
 *   permutation.  That is the from-scratch result whenever the list decodes to its own distinct ids (not for the reference's lossy
 *   cases -- duplicates, a power-of-two maximum under VIDC_PREC_REFERENCE, more than 65 536 ids -- nor for a `b` built with another
 *   precision mode, which the call cannot check): the caveat the append states for the lists a batch does not touch.  Every other
 *   non-empty list is decoded on both sides and re-encoded.
 * d_src (device int64[ntotal_new], may be NULL): every element is written and nothing outside is.  For position q of the new object's
 *   decode_all order it holds p >= 0 if the entry is position p of a's decode_all order, and ~p (negative) if it is position p of
 *   b's: a caller that keeps per-entry payload builds the new payload with one gather.  With a == b the two halves are told apart by
 *   the sign in the same way.
 * Status.  NULL ctx / a / b / out, nlist(a) != nlist(b), either object on another device than ctx, ntotal(a) + ntotal(b) >= 2^32 - 1,
 *   a bad precision_mode or width: VIDC_ERR_INVALID before any device work.  A graph object (rows, Elias-Fano arena) on either side:
 *   VIDC_ERR_UNSUPPORTED.  A merged ROC list above VIDC_ROC_MAX_LIST, a shifted id >= 2^31 (ROC), a shifted id that does not fit
 *   `bits` (packed bits) or 64 bits: VIDC_ERR_DOMAIN.  On any error *out == NULL, both sources are untouched and the context stays
 *   usable.  Two empty objects, or an empty b, give an object equal to a (the wavelet tree is built from ntotal alone: there the result
 *   equals the build).
 * Residency.  No id payload crosses PCIe (vidc_ctx_d2h_bytes does not move), and nothing is sorted: both sides are grouped by list
 *   already.  The new offsets are the sum of the two offset arrays; every list of b goes behind the same list of a as one segmented
 *   copy, a wavefront per 1024-id chunk, add_id added on the way.  Packed bits, Elias-Fano and the wavelet tree are REBUILT:
 *   decode_all of both objects into scratch (once when a == b), the placement, the device-offsets encoder; one 8-byte read-back (the
 *   largest id of b, for the domain checks), no O(nlist) array on the host.  ROC is SPLICED: the lists are classified on the device,
 *   the numbers and merged sizes of the re-encoded ones are read back once (8 bytes per such list), only those are decoded and
 *   encoded, every other list's stream is copied from whichever object holds it.  d_src is arithmetic on the three offset arrays
 *   (packed bits, wavelet tree) or read off the new object's permutation (Elias-Fano, ROC).  The only atomic is the maximum of the
 *   domain check, which does not depend on the order of its operands: no atomic decides a position, nothing spins, the result is the
 *   same on every run.  The calls synchronise; vidc_ctx_last_kernel_ms is the sum over the call's kernels.
 * Out of scope: segmented ROC objects, sharded objects and graph objects; emptying `b` as Faiss does.  (The inverse, Faiss's
 *   copy_subset_to, is the "subset" section behind the remove.) */
int vidc_packed_merge_dev(vidc_ctx *ctx, const vidc_packed *a, const vidc_packed *b, uint64_t add_id, int bits, vidc_packed **out,
                          int64_t *d_src);
int vidc_ef_merge_dev(vidc_ctx *ctx, const vidc_ef *a, const vidc_ef *b, uint64_t add_id, uint32_t flags, vidc_ef **out, int64_t *d_src);
int vidc_wt_merge_dev(vidc_ctx *ctx, const vidc_wt *a, const vidc_wt *b, uint64_t add_id, vidc_wt **out, int64_t *d_src);
int vidc_roc_merge_dev(vidc_ctx *ctx, const vidc_roc *a, const vidc_roc *b, uint64_t add_id, int precision_mode, uint32_t flags,
                       vidc_roc **out, int64_t *d_src);

/* ---------------------------------------------------- remove (batches of pairs, device-resident) */
/* Objects stay immutable: a remove returns a NEW object in *out, the old one stays valid and unchanged, and either may be destroyed
 * first (the new object owns all of its memory).
 *
 * The batch.  Pair i is (d_list_nos[i], d_ids[i]); n_rm < 2^32 - 1.  d_list_nos chooses the mode:
 *   Pairs mode (d_list_nos != NULL): an entry of list l is removed iff some pair has that list number and an id equal to the entry's
 *     id.  A negative list number is skipped and not counted; a list number >= nlist is skipped and counted in *d_invalid.
 *   Any-list mode (d_list_nos == NULL): an entry of ANY list is removed iff its id equals some d_ids[i] -- Faiss's remove_ids over an
 *     IDSelectorBatch.
 *   Equality is over all 64 bits of what the old object decodes to.  Every copy of a matching id inside a list goes; repeated pairs are
 *   harmless.  A valid pair that matches no entry adds one to *d_missing -- in pairs mode that includes an id that sits in another
 *   list, and everywhere an id wider than the object can hold (>= 2^32 for ROC, >= 2^bits for packed bits); a repeated pair is judged
 *   like its first copy.  d_missing and d_invalid are device uint64 the caller zeroes; either may be NULL.
 * The result.  With old_l = list l of the old object in the object's own order (what vidc_*_decode_lists returns) and S_l = old_l
 *   without the removed entries, order kept, the new object is the one the existing encoder builds from the CSR form of S, word for
 *   word (streams, per-list metadata, sizes, compressed_bytes, and the permutation when the flag asks for it, which is over positions
 *   in S_l): vidc_packed_encode with the object's own width, vidc_ef_encode with `flags`, vidc_roc_encode with `precision_mode` and
 *   `flags` (the caller passes the mode the object was built with; the call cannot check it).  A ROC list that loses no entry keeps
 *   its stream and gets the identity permutation: that is the from-scratch result whenever the list decodes to its own distinct ids
 *   (not for the reference's lossy cases -- duplicates, a power-of-two maximum under VIDC_PREC_REFERENCE, more than 65 536 ids).
 *   Lists may become empty, and so may the object.  n_rm == 0, or a batch that matches nothing, returns an object equal to the old one.
 * d_removed (device uint8[ntotal_old], may be NULL): every byte is written -- 1 where the entry at that position of the old object's
 *   decode_all order was removed, 0 elsewhere.  A caller that keeps per-entry payload (the vector codes) drops the same rows.
 * Arrays are device arrays on the context's device, read and written in order on the context's stream.
 * Status.  NULL context, object or out, NULL d_ids with n_rm > 0, n_rm >= 2^32 - 1, a bad precision_mode: VIDC_ERR_INVALID before any
 *   device work.  A graph object (rows, Elias-Fano arena): VIDC_ERR_UNSUPPORTED.  On any error *out == NULL, the old object is
 *   untouched and the context stays usable.
 * Residency.  No id payload crosses PCIe (vidc_ctx_d2h_bytes does not move).  The batch is sorted by (list, id) on the device; every
 *   decoded entry binary-searches its list's run, and the survivors are placed by a scan of per-chunk kill counts: no atomic decides
 *   a position, the result is the same on every run.  Packed bits and Elias-Fano are REBUILT: decode_all into scratch, the mark, the
 *   compaction, the device-offsets encoder; one 8-byte read-back (the survivor count).  ROC is SPLICED: the candidates -- the
 *   non-empty lists a valid pair names; in any-list mode EVERY non-empty list, which decodes the whole object -- are decoded and
 *   marked (their numbers are read back once, 4 bytes each); only the lists that lose an entry are re-encoded (their numbers and
 *   survivor counts are read back, 8 bytes per touched list); every other list's stream is copied.  The calls synchronise;
 *   vidc_ctx_last_kernel_ms is the sum over the call's kernels.
 * There is no wavelet-tree form (a wavelet tree holds a permutation of 0 .. ntotal - 1, which a removal breaks).  The sharded form is
 *   vidc_remove_sharded_dev, behind the sharded append. */
int vidc_packed_remove_dev(vidc_ctx *ctx, const vidc_packed *p, uint64_t n_rm, const int64_t *d_list_nos, const uint64_t *d_ids,
                           vidc_packed **out, uint8_t *d_removed, uint64_t *d_missing, uint64_t *d_invalid);
int vidc_ef_remove_dev(vidc_ctx *ctx, const vidc_ef *e, uint64_t n_rm, const int64_t *d_list_nos, const uint64_t *d_ids,
                       uint32_t flags, vidc_ef **out, uint8_t *d_removed, uint64_t *d_missing, uint64_t *d_invalid);
int vidc_roc_remove_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t n_rm, const int64_t *d_list_nos, const uint64_t *d_ids,
                        int precision_mode, uint32_t flags, vidc_roc **out, uint8_t *d_removed, uint64_t *d_missing, uint64_t *d_invalid);

/* ---------------------------------------------------- subset (a part of every list, chosen by rule, device-resident) */
/* Faiss's InvertedLists::copy_subset_to(other, subset_type, a1, a2), the inverse of the merge: an index is split into shards by id
 * range, id residue, list range or list fraction, and vidc_*_merge_dev puts the shards back together.  Objects stay immutable: a subset
 * returns a NEW object over the same nlist lists in *out, the source stays valid and unchanged, and either may be destroyed first (the
 * new object owns all of its memory).
 *
 * Notation.  old_l = list l of the object in the object's own order (what vidc_*_decode_lists returns), n = |old_l|, off[] = the
 *   object's offsets, T = ntotal.  Ids and all arithmetic are unsigned 64-bit.
 * Which entries are taken.  Entry i of list l, holding `id`, is taken iff
 *     VIDC_SUBSET_ID_RANGE (0)          a1 <= id < a2
 *     VIDC_SUBSET_ID_MOD (1)            id % a1 == a2                                        (needs a1 >= 1, a2 < a1)
 *     VIDC_SUBSET_ELEMENT_RANGE (2)     i1 <= i < i2 with i1 = floor(off[l + 1] * a1 / T) - floor(off[l] * a1 / T) and i2 the same
 *                                       with a2                                              (needs a1 <= a2 <= T)
 *     VIDC_SUBSET_INVLIST_FRACTION (3)  floor(n * a2 / a1) <= i < floor(n * (a2 + 1) / a1)   (needs 1 <= a1 < 2^32, a2 < a1)
 *     VIDC_SUBSET_INVLIST (4)           a1 <= l < a2                  (bounds above nlist are clamped; a1 >= a2 takes nothing)
 *   Type 2: the bounds are local offsets computed from running totals, so i1 may exceed i2, and then nothing is taken from that list
 *   (offsets 0, 3, 4, 10 with a1 = 3, a2 = 4 give list 1 i1 = 1, i2 = 0); i2 <= n always holds under the stated condition; all
 *   products fit 64 bits because T < 2^32.  T == 0 returns an empty object for every type.
 * The result.  With S_l = the taken entries of old_l, order kept, the new object is the one the existing encoder builds from the CSR
 *   form of S, word for word (streams, per-list metadata, sizes, compressed_bytes, and the permutation when the flag asks for it, which
 *   is over positions in S_l): vidc_packed_encode with the object's own width, vidc_ef_encode with `flags`, vidc_roc_encode with
 *   `precision_mode` and `flags` (the caller passes the mode the object was built with; the call cannot check it).  A ROC list that
 *   keeps every entry keeps its stream and gets the identity permutation: that is the from-scratch result whenever the list decodes
 *   to its own distinct ids (not for the reference's lossy cases -- duplicates, a power-of-two maximum under VIDC_PREC_REFERENCE, more
 *   than 65 536 ids), the caveat the remove states.  A list that keeps nothing becomes empty without any decode.
 * d_taken (device uint8[T], may be NULL): every byte is written -- 1 where the entry at that position of the source's decode_all order
 *   is in the subset, 0 elsewhere; nothing outside the T bytes is written.  A caller that keeps per-entry payload (the vector codes)
 *   takes the same rows.  *n_taken (host, may be NULL) = the size of the subset.
 * Status.  NULL ctx / object / out, a subset_type outside 0 .. 4, an argument condition above violated, a bad precision_mode:
 *   VIDC_ERR_INVALID before any device work.  A graph object (rows, Elias-Fano arena): VIDC_ERR_UNSUPPORTED.  On any error
 *   *out == NULL, the source is untouched and the context stays usable.
 * Residency.  No id payload crosses PCIe (vidc_ctx_d2h_bytes, which counts id payload, does not move: what comes back are counts and
 *   list numbers).  Types 0 and 1 evaluate the predicate on the decoded ids, a wavefront per 1024-id chunk, and place the taken entries
 *   by a scan of per-chunk counts as a remove places its survivors; for ID_MOD a power-of-two a1 is a mask and a1 < 2^32 reduces the
 *   high half of the id first.  Types 2 .. 4 need no mark: one thread per list computes [i1, i2) from the offsets alone, a scan gives
 *   the new offsets and a segmented copy takes old_l[i1:i2] to its place.  Packed bits and Elias-Fano are REBUILT: decode_all into
 *   scratch, the mark and the compaction or the slice, the device-offsets encoder; one 8-byte read-back (the size of the subset).  ROC is
 *   SPLICED: type 4 decodes nothing -- every kept list's stream is copied, the other lists are empty; types 2 and 3 decode, slice and
 *   re-encode only the lists that keep a part (the host finds them on its mirror of the offsets); types 0 and 1 take every non-empty
 *   list as a candidate, as the remove's any-list mode does -- lists that keep everything keep their stream, the others are re-encoded
 *   (their numbers and sizes are read back, 8 bytes per such list).  No atomic decides a position, nothing spins, the result is the
 *   same on every run.  The calls synchronise; vidc_ctx_last_kernel_ms is the sum over the call's kernels.
 * There is no wavelet-tree form (a wavelet tree holds a permutation of 0 .. ntotal - 1, which a subset breaks).  Segmented ROC objects
 *   and sharded objects are out of scope. */
#define VIDC_SUBSET_ID_RANGE 0
#define VIDC_SUBSET_ID_MOD 1
#define VIDC_SUBSET_ELEMENT_RANGE 2
#define VIDC_SUBSET_INVLIST_FRACTION 3
#define VIDC_SUBSET_INVLIST 4
int vidc_packed_subset_dev(vidc_ctx *ctx, const vidc_packed *p, int subset_type, uint64_t a1, uint64_t a2, vidc_packed **out,
                           uint8_t *d_taken, uint64_t *n_taken);
int vidc_ef_subset_dev(vidc_ctx *ctx, const vidc_ef *e, int subset_type, uint64_t a1, uint64_t a2, uint32_t flags, vidc_ef **out,
                       uint8_t *d_taken, uint64_t *n_taken);
int vidc_roc_subset_dev(vidc_ctx *ctx, const vidc_roc *r, int subset_type, uint64_t a1, uint64_t a2, int precision_mode, uint32_t flags,
                        vidc_roc **out, uint8_t *d_taken, uint64_t *n_taken);

/* ---------------------------------------------------- locate (batches of pairs, device-resident) */
/* The inverse of translate_labels -- Faiss's direct map (DirectMap, reconstruct, update_vectors): at which (list, offset) does an id
 * sit?  The object is read-only and unchanged.
 *
 * The batch is the remove's.  Pair i is (d_list_nos[i], d_ids[i]); n < 2^32 - 1.  d_list_nos chooses the mode:
 *   Pairs mode (d_list_nos != NULL): the id is looked for in list d_list_nos[i] only.  A negative list number is skipped and not
 *     counted; a list number >= nlist is skipped and counted in *d_invalid.
 *   Any-list mode (d_list_nos == NULL): the id is looked for in every list.
 *   Equality is over all 64 bits of what the object decodes to.  An id the object cannot hold matches nothing: >= 2^32 for ROC,
 *   >= 2^bits for packed bits, >= ntotal for the wavelet tree.
 * The result.  d_labels (device int64[n]): every element is written and nothing outside is.  d_labels[i] = list_no << 32 | offset of
 *   an entry equal to d_ids[i], the offset in the object's own order (what vidc_*_decode_lists and translate_labels use: sampling
 *   order for ROC, ascending for Elias-Fano and the wavelet tree, input order for packed bits).  If several entries match, the label
 *   is the smallest one: lowest list, then lowest offset -- the same on every run.  No match, a skipped or an invalid pair: -1.
 *   *d_missing += the valid pairs that got -1 (in pairs mode that includes an id that sits in another list); repeated pairs each count
 *   and each get the same label.  d_missing and d_invalid are device uint64 the caller zeroes; either may be NULL.  Wherever
 *   d_labels[i] >= 0, vidc_*_translate_labels_dev on the same object maps it back to d_ids[i].  d_labels must not overlap the inputs.
 * Arrays are device arrays on the context's device, read and written in order on the context's stream.
 * Status.  NULL context or object, NULL d_ids or d_labels with n > 0, n >= 2^32 - 1: VIDC_ERR_INVALID before any device work.  A graph
 *   object (rows, Elias-Fano arena): VIDC_ERR_UNSUPPORTED.  n == 0: VIDC_OK, nothing is launched.  The context stays usable after any
 *   error.
 * Residency.  No id payload crosses PCIe (vidc_ctx_d2h_bytes does not move).  Packed bits, Elias-Fano, ROC: the batch is sorted by
 *   (list, id) as a remove sorts it, the object is decoded into scratch (decode_all; ROC: the candidates of a remove -- the non-empty
 *   lists a valid pair names, in any-list mode EVERY non-empty list, which decodes the whole object), every decoded entry
 *   binary-searches its list's run and a 64-bit atomic minimum keeps the smallest label per batch value: a minimum does not depend on
 *   the order of its operands, nothing timing-dependent decides a result.  Packed bits and Elias-Fano read nothing back; ROC reads
 *   back the candidate list numbers once (4 bytes each).  These calls wait for their last kernel; vidc_ctx_last_kernel_ms is the sum
 *   over the call's kernels.  The wavelet tree walks every id down its levels (the bit at the position, the rank inside the node): a
 *   thread per pair, no sort, no decode, enqueue only like vidc_wt_translate_labels_dev (vidc_ctx_last_kernel_ms is left alone).
 * Out of scope: segmented ROC objects, sharded objects and graph objects; a search inside compressed Elias-Fano lists; a persistent
 *   direct map kept beside the object.  (The search inside compressed Elias-Fano lists is vidc_ef_rank_dev, below.) */
int vidc_packed_locate_dev(vidc_ctx *ctx, const vidc_packed *p, uint64_t n, const int64_t *d_list_nos, const uint64_t *d_ids,
                           int64_t *d_labels, uint64_t *d_missing, uint64_t *d_invalid);
int vidc_ef_locate_dev(vidc_ctx *ctx, const vidc_ef *e, uint64_t n, const int64_t *d_list_nos, const uint64_t *d_ids,
                       int64_t *d_labels, uint64_t *d_missing, uint64_t *d_invalid);
int vidc_wt_locate_dev(vidc_ctx *ctx, const vidc_wt *w, uint64_t n, const int64_t *d_list_nos, const uint64_t *d_ids,
                       int64_t *d_labels, uint64_t *d_missing, uint64_t *d_invalid);
int vidc_roc_locate_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t n, const int64_t *d_list_nos, const uint64_t *d_ids,
                        int64_t *d_labels, uint64_t *d_missing, uint64_t *d_invalid);

/* ---------------------------------------------------- rank inside Elias-Fano lists and rows (device-resident) */
/* How many entries of list d_list_nos[i] are smaller than d_ids[i]?  Answered inside the compressed streams: nothing is decoded.  From
 * the rank follow membership, the successor (next_geq), a count of ids in a range, and for graph rows has_edge(u, v).
 *
 * Inputs.  All arrays are device arrays on the context's device, read and written in order on the context's stream.  Pair i asks
 *   about list d_list_nos[i] (graph objects: the node).  Pairs mode only: d_list_nos is required.  A negative list number is skipped
 *   and not counted; a list number >= nlist is skipped and counted in *d_invalid (device uint64 the caller zeroes, may be NULL).
 * The result.  d_ranks[i] = r, the number of entries of that list < d_ids[i], compared over all 64 bits, unsigned: 0 <= r <= size.  r
 *   is the offset of the first entry >= the id in the object's own (ascending) order: where r < size, list << 32 | r is a label that
 *   vidc_ef_translate_labels_dev maps to the successor; of equal entries r is the first (vidc_ef_locate_dev's smallest label).  An id
 *   above the list's largest gives r = size (ids >= 2^32, 2^63 and 2^64 - 1 are legal queries); an empty list gives 0; skipped and
 *   invalid pairs get -1.  Every element of d_ranks is written and nothing outside it.  d_found (device uint8[n], may be NULL):
 *   d_found[i] = 1 iff r < size and entry r equals the id, else 0 (also for skipped pairs); every element is written.  The outputs
 *   must not overlap the inputs.
 * Status.  NULL context or object, NULL d_list_nos, d_ids or d_ranks with n > 0, n >= 2^32 - 1: VIDC_ERR_INVALID before any device
 *   work.  n == 0: VIDC_OK, nothing is launched.  The context stays usable after any error.
 * Residency.  Enqueue only, like vidc_wt_locate_dev: no wait, no read-back; vidc_ctx_d2h_bytes does not move and
 *   vidc_ctx_last_kernel_ms is left alone.  No allocation at all, so none that grows with ntotal.  The object is not changed.
 * Objects.  Every Elias-Fano object: lists (per-list streams and the select directory: 16 lanes per pair binary-search the directory
 *   for the batch of 64 high words that holds a zero of the unary high stream, scan that batch's popcounts, and binary-search the
 *   bucket's low fields), graph rows of more than 64 edges (the same, list = node), and graph rows of up to 64 edges, read in place
 *   from the fixed-stride arena by one lane per pair (the per-list streams are NOT built for this call). */
int vidc_ef_rank_dev(vidc_ctx *ctx, const vidc_ef *e, uint64_t n, const int64_t *d_list_nos, const uint64_t *d_ids, int64_t *d_ranks,
                     uint8_t *d_found, uint64_t *d_invalid);

/* ---------------------------------------------------- search graph rows (device-resident, one launch) */
/* Best-first search over a neighbour graph (NSG search_on_graph) for a batch of queries as ONE kernel launch: every query gets a
 * wavefront of its own, which decodes the compressed rows it expands inside the kernel; the pool, the frontier and the visited set
 * never leave the device.  vidc_rows_search_dev takes raw rows (int32 [N, K], the uncompressed baseline), the other two the objects
 * of vidc_compact_rows_encode and vidc_ef_encode_rows.
 *
 * Semantics (per query, independently; graph_search.search of the Python package is the statement).  The pool holds at most L entries
 *   (distance, node, expanded) ordered by (distance, node) ascending and starts as the entry node alone.  A step takes the first
 *   unexpanded entry, marks it expanded and reads its row; every neighbour not yet visited is marked visited, gets its distance and
 *   is inserted; the best L stay.  The search ends when no unexpanded entry is left or after max_rounds steps (0: no cap).  Visited
 *   is permanent (a node dropped from the pool stays visited); a neighbour that a row holds twice counts once.  Distances are
 *   squared L2 in float32.  Ties in distance are decided by the node id, so the result does not depend on the order of a row.
 * Arrays.  All device arrays on the context's device.  d_x: float32 [N, d] row-major; d_xq: float32 [nq, d]; d_D float32 / d_I int64:
 *   [nq, k], the first k pool entries of every query, padded with +inf / -1: every element is written and nothing outside them.
 *   d_stats (may be NULL): uint32 [nq, 2] = {steps taken, distances computed (the entry's included)}.
 * Rows.  A raw row ends at its first negative entry, a compact row at its first sentinel, an Elias-Fano row is its n ids.  A decoded
 *   id >= N is skipped: it is never used as an index into d_x or the visited set, so a damaged image gives a wrong result, not an
 *   access outside the call's arrays.
 * Status.  VIDC_ERR_INVALID before any device work: NULL context or object, NULL arrays with nq > 0, anything outside
 *   1 <= k <= L <= 256, 1 <= d <= 2048, entry < N, N < 2^31, nq < 2^32 - 1 (raw rows: K >= 1).  nq == 0: VIDC_OK, nothing is
 *   launched.  VIDC_ERR_UNSUPPORTED: an Elias-Fano object that holds lists and not graph rows; a graph object of rows wider than 64
 *   edges (it has no fixed-stride arena); compact rows outside the K limits of vidc_compact_rows_encode.
 * Scratch.  The visited set is exact: a bitset of N bits per RESIDENT WAVEFRONT (slot), not per query, taken from the context's
 *   block cache: slots * ceil(N / 64) * 8 bytes with slots = min(nq, 32 * compute units, 1024) -- at most 128 MB at N = 10^6.  A slot
 *   is cleared by its wavefront in front of every query (a wide memset inside the kernel, measured at 12-14 % of the kernel's time at most on a
 *   10^6-node graph; replaying a log of the visited nodes instead was not built).
 * Residency.  Enqueued on the context's stream; the call waits for its kernel, because the scratch goes back to the cache.
 *   vidc_ctx_d2h_bytes does not move; vidc_ctx_last_kernel_ms is the kernel's time.  The objects are not changed; the Elias-Fano
 *   arena is read in place (the per-list streams are not built for this call).
 * Not here.  There is no ROC form: a ROC row is one serial ANS chain, which a single lane of the query's wavefront would have to
 *   run -- the batched search over vidc_roc_decode_rows_dev (graph_search.search_batched) stays the ROC path.  Inner product,
 *   per-query entry nodes and sharded graphs are out of scope as well. */
int vidc_rows_search_dev(vidc_ctx *ctx, uint64_t N, uint32_t K, const int32_t *d_rows, const float *d_x, uint32_t d, uint64_t nq,
                         const float *d_xq, uint32_t k, uint32_t L, uint32_t entry, uint32_t max_rounds, float *d_D, int64_t *d_I,
                         uint32_t *d_stats);
int vidc_compact_search_dev(vidc_ctx *ctx, const vidc_compact *c, const float *d_x, uint32_t d, uint64_t nq, const float *d_xq,
                            uint32_t k, uint32_t L, uint32_t entry, uint32_t max_rounds, float *d_D, int64_t *d_I, uint32_t *d_stats);
int vidc_ef_search_dev(vidc_ctx *ctx, const vidc_ef *e, const float *d_x, uint32_t d, uint64_t nq, const float *d_xq, uint32_t k,
                       uint32_t L, uint32_t entry, uint32_t max_rounds, float *d_D, int64_t *d_I, uint32_t *d_stats);

/* ---------------------------------------------------- scan IVF lists (device-resident, deferred id decoding) */
/* The scan of the IVF search with deferred id decoding (custom_invlists_impl.cpp:407-526) for a batch of queries on the device: every
 * probed list of a query is scanned and the k best (distance, list_no << 32 | offset) labels stay.  D and the labels are device
 * arrays: vidc_*_translate_labels_dev turns the labels into ids without a host trip.
 *
 * Semantics (per query, independently; tests/ivf_scan_ref.py is the statement).  The candidates are all entries of the DISTINCT VALID
 *   lists the query's probe row names: a probe that is negative or >= nlist is skipped (Faiss writes -1 for "no list"), a list named
 *   twice in a row is scanned once.  The distance is squared L2 in float32: VIDC_IVF_FLAT, query minus stored vector; VIDC_IVF_PQ8, the
 *   sum over the M sub-quantisers of || xq_m - codebook[m][code_m] ||^2 (asymmetric distance from a per-query table; the value of
 *   decoding the code and taking L2).  The result is the first k candidates in ascending (distance, label) order, label =
 *   list_no << 32 | offset, padded with +inf / -1.  Ties are decided by the label, so the result does not depend on how the work was cut.
 * Arrays.  All device arrays on the context's device.  d_offsets: uint64 [nlist + 1]; d_codes: uint8 [ntotal, code_size] in the
 *   container's order (code_size = 4 * d, or M); d_codebooks (PQ8): float32 [M, 256, d / M]; d_xq: float32 [nq, d]; d_probes: int64
 *   [nq, nprobe]; d_D float32 / d_labels int64: [nq, k] -- every element is written and nothing outside them.  d_stats (may be NULL):
 *   uint32 [nq, 2] = {lists scanned, codes scanned}.  The inputs are not changed.
 * Bounds.  A list's range is clamped to a <= b <= ntotal before it indexes d_codes, and a PQ code byte indexes a 256-entry table:
 *   damaged offsets give a wrong result, never a read outside the call's arrays.
 * Status.  VIDC_ERR_INVALID before any device work, nothing written: NULL context; NULL arrays with nq > 0; k outside 1 .. 256; nprobe
 *   outside 1 .. 1024; d outside 1 .. 2048; ntotal >= 2^32 (a key packs a position in 32 bits); nlist >= 2^31; an unknown code_kind;
 *   PQ8 with M outside 1 .. 64, with d % M != 0, or with NULL codebooks.  nq == 0: VIDC_OK, nothing is launched.
 * What runs.  A wavefront per (query, piece): small batches still fill the device because a probe row is cut into S of 1, 2, 4, 8, 16
 *   contiguous pieces -- the smallest S with nq * S >= the resident wavefronts, S <= nprobe; the row is de-duplicated before the cut.
 *   With S > 1 a second kernel merges the pieces' sorted runs, a wavefront per query.
 * Scratch.  None with S == 1.  Otherwise nq * S * (k + 1) * 8 bytes from the context's block cache (the pieces' keys [nq, S, k] and
 *   their counters): at most 16 * 257 * 8 bytes per query, and S > 1 only while nq is below the resident wavefronts (<= 8192).
 * Residency.  Enqueued on the context's stream; the call waits for its kernels.  vidc_ctx_d2h_bytes does not move;
 *   vidc_ctx_last_kernel_ms is the kernels' time.
 * Not here.  Inner product, residual PQ, sub-quantisers of other than 8 bits, returning the codes (return_codes), the coarse
 *   quantiser (the caller brings the probes), sharded and segmented containers.  The Faiss adapter does not call this: Faiss's own
 *   scanner stays its path.  (Residual PQ has entry points of its own: see the residual section behind the range search.) */
#define VIDC_IVF_FLAT 0 /* code = d float32, code_size = 4 * d */
#define VIDC_IVF_PQ8 1  /* code = M bytes, codebooks float32 [M, 256, d / M] */
int vidc_ivf_scan_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes, int code_kind,
                      uint32_t d, uint32_t M, const float *d_codebooks, uint64_t nq, const float *d_xq, uint32_t nprobe,
                      const int64_t *d_probes, uint32_t k, float *d_D, int64_t *d_labels, uint32_t *d_stats);

/* ---------------------------------------------------- range search over IVF lists (device-resident, deferred id decoding) */
/* IndexIVF::range_search's scan for a batch of queries on the device: every entry of a query's probed lists whose distance is below
 * a radius, as (distance, list_no << 32 | offset).  The result has a variable length, so there are two calls and the caller allocates
 * between them: count -> the limits of every slot and the total; fill -> D and the labels.  vidc_*_translate_labels_dev turns the
 * labels into ids: only what passed the radius is decoded.  A top-k scan at k = 256 is no substitute: it truncates.
 *
 * Semantics (tests/ivf_range_ref.py is the statement).  The arguments up to d_probes are vidc_ivf_scan_dev's, with its arrays.
 *   Slot s = q * nprobe + j is entry j of query q's probe row.  Its candidates are the entries of the list it names, in ascending
 *   offset order, if the entry is a valid list number and the FIRST mention of that list in the row (the probe rules of the scan: a
 *   probe that is negative or >= nlist is skipped, a repeated list counts once); every other slot has no candidates.  A candidate is a
 *   hit iff distance < radius, compared strictly in float32 as Faiss's L2 range search does; the distances are the scan's, bit for bit
 *   (VIDC_IVF_FLAT and VIDC_IVF_PQ8).  A NaN, zero or negative radius gives no hit, +inf gives every candidate.
 * Count.  d_slot_lims: device uint64 [nq * nprobe + 1], the exclusive prefix sum of the hits per slot in slot order, every element
 *   written; d_slot_lims[nq * nprobe] is the total, copied to *total (HOST) unless total is NULL.  Query q's results are
 *   [d_slot_lims[q * nprobe], d_slot_lims[(q + 1) * nprobe]): Faiss's lims is the strided view d_slot_lims[::nprobe].
 * Fill.  The r-th hit of slot s goes to position d_slot_lims[s] + r of d_D (float32) / d_labels (int64), device arrays of `capacity`
 *   entries, label = list_no << 32 | offset.  The order is probe-row order, then offset: it does not depend on how the work was cut,
 *   and no atomic operation decides a position.  With the d_slot_lims of a count over the same arguments and capacity >= the total,
 *   every position below the total is written.
 * Bounds.  The fill writes position p of slot s only if p < d_slot_lims[s + 1] and p < capacity; list ranges are clamped as in the
 *   scan.  A d_slot_lims that came from another radius, a capacity below the total or damaged offsets give a wrong or partial
 *   result, never a write outside [0, capacity) of the two output arrays nor a read outside the call's arrays.  Positions of a slot
 *   beyond the hits the fill finds are left untouched.
 * Status.  VIDC_ERR_INVALID before any device work, nothing written: every refusal of vidc_ivf_scan_dev but k's (there is no k);
 *   nq * nprobe >= 2^32 - 1; NULL d_slot_lims with nq > 0; NULL d_D or d_labels with capacity > 0.  nq == 0: VIDC_OK; the count writes
 *   d_slot_lims[0] = 0 if the array is given and *total = 0 if total is given, the fill launches nothing.  capacity == 0: VIDC_OK,
 *   nothing written.
 * What runs.  One kernel per call, a wavefront per (query, piece) with the cut of the scan; the pieces of a query own disjoint slots,
 *   so there is no merge.  Count: the hit ballots are summed per slot, then one device scan of the counts.  Fill: the distance pass
 *   again (the function and the plan of the count, hence the same bits), every hit stored at its place.
 * Scratch.  nq * nprobe uint32 hit counts from the context's block cache, and the tile sums of the device scan beyond 8192 slots.
 *   Nothing grows with the number of results.
 * Residency.  Enqueued on the context's stream; both calls wait for their kernels.  The count with total != NULL reads back exactly 8
 *   bytes (vidc_ctx_d2h_bytes moves by 8), with total == NULL nothing; the fill never moves it.  vidc_ctx_last_kernel_ms is the
 *   call's kernels' time.
 * Not here.  Per-query radii; inner product, residual PQ, sub-quantisers of other than 8 bits; the coarse quantiser (the caller
 *   brings the probes); sharded containers; a one-pass form that buffers hits; the Faiss adapter (Faiss's own scanner stays its
 *   path).  (Residual PQ has entry points of its own: see the residual section below.) */
int vidc_ivf_range_count_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                             int code_kind, uint32_t d, uint32_t M, const float *d_codebooks, uint64_t nq, const float *d_xq,
                             uint32_t nprobe, const int64_t *d_probes, float radius, uint64_t *d_slot_lims, uint64_t *total);
int vidc_ivf_range_fill_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                            int code_kind, uint32_t d, uint32_t M, const float *d_codebooks, uint64_t nq, const float *d_xq,
                            uint32_t nprobe, const int64_t *d_probes, float radius, const uint64_t *d_slot_lims, uint64_t capacity,
                            float *d_D, int64_t *d_labels);

/* ---------------------------------------------------- residual PQ in the IVF scan and range search (by_residual, device-resident) */
/* vidc_ivf_scan_dev and the two range calls for the index faiss.index_factory(d, "IVF<n>,PQ<M>") builds: an IndexIVFPQ with
 * by_residual = true, where the code of a vector is the 8-bit PQ code of (vector - its list's centroid).  There is no code_kind
 * argument: codes are M bytes each.  d_centroids: device float32 [nlist, d]; every other argument is the one of the same name in
 * vidc_ivf_scan_dev / vidc_ivf_range_count_dev / vidc_ivf_range_fill_dev, with its array.
 *
 * Semantics (tests/ivf_residual_ref.py is the statement, csrc/ivf_residual_ref.h the serial form).  For a query xq, a valid list l
 *   and a code of M bytes in that list, with dsub = d / M:
 *     r           = xq - centroids[l]                                   one float32 subtraction per component
 *     entry(m, c) = sum_i (r[m * dsub + i] - codebooks[m][c][i])^2      float32, components in order
 *     distance    = sum_m entry(m, code[m])                             float32, in m order
 *   the form Faiss uses without a precomputed table: a distance table per (query, list).  Everything else is unchanged from the
 *   calls above: invalid probes are skipped and a repeated list counts once; a list's range is clamped; the key is
 *   (distance bits << 32 | position); the scan's result is the first k in ascending (distance, label) order, padded with +inf / -1;
 *   d_stats = {lists scanned, codes scanned}, an empty list still a list; a range hit is distance < radius, strictly; the slot
 *   limits, the order of range results and the bounds on what the fill writes.  The distances of the two range calls are the
 *   scan's, bit for bit: one function builds the table and one runs the trip, for all three.
 * Bounds.  A centroid row is read only for a list number the probe rule accepted (0 <= l < nlist); a list's range is clamped to
 *   a <= b <= ntotal before it indexes d_codes; a code byte indexes a 256-entry table.  Damaged offsets give a wrong result, never
 *   an access outside the call's arrays.
 * Status.  VIDC_ERR_INVALID before any device work, nothing written: the refusals of the call above it for VIDC_IVF_PQ8 (NULL
 *   context; NULL arrays with nq > 0; k outside 1 .. 256; nprobe outside 1 .. 1024; d outside 1 .. 2048; ntotal >= 2^32; nlist >=
 *   2^31; M outside 1 .. 64; d % M != 0; NULL codebooks; for the range calls nq * nprobe >= 2^32 - 1, NULL d_slot_lims with nq > 0,
 *   NULL d_D or d_labels with capacity > 0), and NULL d_centroids with nq > 0.  nq == 0 and capacity == 0 behave as they do there.
 * What runs.  The kernels of the calls above with one step more: a wavefront per (query, piece), the same cut S, pools, insert by
 *   rank and merge kernel, count / device scan / fill.  In front of every probed list whose clamped range is not empty the wavefront
 *   writes r to LDS and builds that list's M x 256 table from the codebooks (256 * d * 4 bytes read per (query, list)); an empty list
 *   builds nothing.  Tables belong to lists, so cutting a row into S pieces builds no table twice.
 * LDS.  Per wavefront: the scan's pools (2 * k * 8 + 768 bytes; the range calls have none), the probe row round16(4 * nprobe), the
 *   query vector and the residual 2 * round16(4 * d), the table 1024 * M.  Scan at d = 128, M = 16, k = 20, nprobe = 16: 18560 bytes,
 *   eight wavefronts per compute unit; at the limits (d = 2048, M = 64, nprobe = 1024, k = 256) 90880 bytes, one.
 * Scratch.  That of the calls above: none for an uncut scan, nq * S * (k + 1) * 8 bytes for a cut one; nq * nprobe uint32 hit counts
 *   and the tile sums of the device scan for a count; none for a fill.
 * Residency.  Enqueued on the context's stream; every call waits for its kernels.  vidc_ctx_d2h_bytes does not move, except by the 8
 *   bytes of a count with total != NULL.  vidc_ctx_last_kernel_ms is the call's kernels' time.
 * Not here.  Inner product; precomputed tables (Faiss's use_precomputed_table: its float32 bits would differ); sub-quantisers of
 *   other than 8 bits; per-query radii; the coarse quantiser (the caller brings the probes); sharded containers; the Faiss adapter
 *   (Faiss's own scanner stays its path). */
int vidc_ivf_scan_residual_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                               uint32_t d, uint32_t M, const float *d_codebooks, const float *d_centroids, uint64_t nq,
                               const float *d_xq, uint32_t nprobe, const int64_t *d_probes, uint32_t k, float *d_D,
                               int64_t *d_labels, uint32_t *d_stats);
int vidc_ivf_range_count_residual_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                                      uint32_t d, uint32_t M, const float *d_codebooks, const float *d_centroids, uint64_t nq,
                                      const float *d_xq, uint32_t nprobe, const int64_t *d_probes, float radius,
                                      uint64_t *d_slot_lims, uint64_t *total);
int vidc_ivf_range_fill_residual_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint8_t *d_codes,
                                     uint32_t d, uint32_t M, const float *d_codebooks, const float *d_centroids, uint64_t nq,
                                     const float *d_xq, uint32_t nprobe, const int64_t *d_probes, float radius,
                                     const uint64_t *d_slot_lims, uint64_t capacity, float *d_D, int64_t *d_labels);

/* ---------------------------------------------------- update rows (graph objects, device-resident) */
/* What an NSG / HNSW-style insert does to its adjacency -- rows for the new nodes, rewritten rows for the neighbours that gained a
 * back-edge -- without re-encoding the graph.  Objects stay immutable: the call returns a NEW object in *out that owns all of its
 * memory; the old one stays valid and unchanged, and either may be destroyed first.
 *
 * The batch.  d_nodes: device int64[m]; d_rows: device int32[m * K], K the object's K, rows -1 terminated; m < 2^32 - 1.  The updated
 *   matrix R' has N_new >= N_old rows of K entries: row v is batch row i for the LARGEST i with d_nodes[i] == v (the last mention wins:
 *   the result is the same on every run); otherwise old row v (what the object's decode_rows returns) for v < N_old; otherwise the
 *   empty row (-1 in column 0).  A negative node is skipped and not counted; a node >= N_new is skipped and counted in *d_invalid (a
 *   device uint64 the caller zeroes; may be NULL).  Arrays are read in order on the context's stream.
 * The result is the object vidc_compact_rows_encode / vidc_ef_encode_rows / vidc_roc_encode_rows(precision_mode) builds from
 *   (N_new, K, R'), in everything that can be exported or decoded -- compact: bits, stride, size_in_bytes and every byte of export_all
 *   (the sentinel is N_new in EVERY row, and the fields re-pack when the width steps); Elias-Fano: list_info, stream_words,
 *   compressed_bytes, every word of export_all, and the arena geometry of a fresh object, sized for max(N_new - 1, the largest id of R');
 *   ROC: list_info (sizes, precisions, heads, nwords, draws), total_words, compressed_bytes, every word of export_all_words.  A ROC
 *   stream depends only on the row's multiset and precision, so an untouched row keeps its stream bit for bit (the caller passes the
 *   precision_mode the object was built with; the call cannot check it).
 * Status.  NULL context, object or out, a NULL array with m > 0, m >= 2^32 - 1, N_new < N_old, N_new >= 2^32 - 1, a bad precision_mode:
 *   VIDC_ERR_INVALID before any device work.  An IVF object (not built by *_encode_rows): VIDC_ERR_UNSUPPORTED.  A wide Elias-Fano or
 *   ROC object (K > 64: these are CSR objects that only carry their K): VIDC_ERR_UNSUPPORTED -- out of scope here; compact rows take
 *   every K their encoder takes (1 .. 4096).  Ids in batch rows follow the encoders: compact, an id outside [0, N_new); Elias-Fano, a
 *   negative id before the terminator; ROC, an id >= 2^31 (a negative int32): VIDC_ERR_DOMAIN.  Compact and Elias-Fano judge the batch
 *   rows that reach R' (a skipped row, or one that loses to a later mention, is not read for content); ROC encodes and therefore judges
 *   every batch row.  On any error *out == NULL, the old object is untouched and the context stays usable.  m == 0 with N_new == N_old
 *   returns an object equal to the old one.
 * What runs.  The slot table (slot[v] = 1 + the largest batch index naming v, one atomicMax per batch entry over a zeroed
 *   uint32[N_new]; the invalid nodes are counted in the same pass), then
 *   compact: ONE re-pack kernel writes every row -- the batch row packed from int32, or the old record's fields re-emitted at the new
 *     width with the sentinel replaced, or the sentinel alone; a 4-byte domain flag comes back;
 *   Elias-Fano: a pass over the rows of R' finds its largest id and checks its domain (8 bytes come back and fix the geometry); the tile
 *     encoder codes the m batch rows into a scratch arena at that geometry; one kernel writes the new arena record by record from
 *     {scratch, old arena, zero}, re-striding old records when (low words, high words) changed; one writes the per-row meta and sums
 *     the totals (1 KiB comes back);
 *   ROC: the m batch rows are encoded by the rows path into a temporary object, and the splice of vidc_roc_regroup runs over {old,
 *     temporary} with the slot table in the place of its host table: metadata gather, one scan launch set, the totals (24 bytes come
 *     back), the chunked 16-byte word copy.  The result carries no planner hints, like an imported object.
 *   No row payload crosses PCIe (vidc_ctx_d2h_bytes does not move), no kernel waits for another workgroup, and every position comes
 *   from a scan or a multiplication.  The calls synchronise; vidc_ctx_last_kernel_ms covers their launches. */
int vidc_compact_update_rows_dev(vidc_ctx *ctx, const vidc_compact *c, uint64_t m, const int64_t *d_nodes, const int32_t *d_rows,
                                 uint64_t N_new, vidc_compact **out, uint64_t *d_invalid);
int vidc_ef_update_rows_dev(vidc_ctx *ctx, const vidc_ef *e, uint64_t m, const int64_t *d_nodes, const int32_t *d_rows, uint64_t N_new,
                            vidc_ef **out, uint64_t *d_invalid);
int vidc_roc_update_rows_dev(vidc_ctx *ctx, const vidc_roc *r, uint64_t m, const int64_t *d_nodes, const int32_t *d_rows, uint64_t N_new,
                             int precision_mode, vidc_roc **out, uint64_t *d_invalid);

/* ---------------------------------------------- sharded lists (several contexts, one process) */
/* One CSR set of lists cut into shards, one codec object per shard, each built and served through its own context: the container of a
 * process that drives all of its GPUs itself (a Faiss process and its OpenMP loops, custom_invlists_impl.cpp:147,508-525), where
 * sharding.py's ShardedInvLists needs one process per GPU.  Contexts of one object may sit on the same device: a supported mode (the host
 * plans several ROC shards at once), and the only one exercised so far -- NOTHING HERE HAS BEEN RUN ON MORE THAN ONE GPU.
 *
 * Ownership.  Shards are balanced by the longest-processing-time rule on the list lengths: lists in descending size, ties by ascending
 *   list number; each to the shard with the least load so far, ties to the lowest shard number (sharding.lpt_partition, bit for bit).
 *   The local number of a list is its rank among its owner's lists in ascending global number.  The map is replicated on the home device
 *   (one uint64 per list: shard << 32 | local_no); nlist < 2^32.
 * Contract.  Shard s holds exactly the object that vidc_{packed,ef,roc}_encode builds from its cut CSR with the same param and flags,
 *   word for word.  kind = VIDC_KIND_PACKED: param = the packed width, 0 = vidc_packed_bits_for(ntotal) of the GLOBAL id count (every shard
 *   uses the same width); VIDC_KIND_ROC: param = precision_mode; VIDC_KIND_EF: param is ignored.  flags are the codec's own
 *   (VIDC_ROC_WANT_PERM, VIDC_EF_WANT_PERM).  A shard that owns no list holds no object and is skipped everywhere; a shard whose lists are
 *   all empty holds an ordinary object.  VIDC_KIND_WT is VIDC_ERR_UNSUPPORTED: a shard's ids are not a permutation of 0 .. n - 1.
 * Contexts.  shard_ctxs: nshards distinct contexts on any devices, repeated devices included; `home` may be one of them.  The caller owns
 *   them and keeps them alive as long as the object.  Device inputs and outputs of every call live on the home device and are read and
 *   written on the home context's stream.  A call drives the home context and every shard context: no other call may use any of them
 *   meanwhile.
 * What runs where.  The cut (global ids -> each shard's contiguous ids), its inverse (decode_all) and the placement of decode_lists
 *   results are one segmented-copy kernel on the home stream (a wavefront per 1024-element chunk of a segment; 16-byte accesses where a
 *   segment's source and destination share their alignment mod 16).  A shard on the home device is read and written in place (blocks of
 *   its context's cache); a shard on another device goes through hipMemcpyAsync(hipMemcpyDefault) between staging blocks of the two
 *   contexts' caches.  Per-shard calls that wait (encode, append, decode_*, perm, ROC's translate) are issued from one host thread per involved
 *   shard, at most VIDC_SHARDS_MAX; each sets its device itself.  The enqueue-only per-shard calls (packed, Elias-Fano translate) are
 *   issued from the calling thread and ordered against the home stream with events the object owns (timing disabled; no spinning kernels,
 *   no cross-context atomics).
 * Errors.  NULL arguments, nshards outside 1 .. VIDC_SHARDS_MAX, a repeated context, an unknown kind: VIDC_ERR_INVALID before any device
 *   work.  A status from a shard is returned; vidc_last_error names the lowest-numbered failing shard and carries its message.  On any
 *   error of an encode *out == NULL, every shard object already built is destroyed, and every context stays usable. */
typedef struct vidc_shards vidc_shards;
#define VIDC_KIND_PACKED 0
#define VIDC_KIND_EF 1
#define VIDC_KIND_ROC 2
#define VIDC_KIND_WT 3 /* known, and refused: VIDC_ERR_UNSUPPORTED */
#define VIDC_SHARDS_MAX 8
int vidc_shards_encode(vidc_ctx *home, int nshards, vidc_ctx *const *shard_ctxs, int kind, int param, uint32_t flags, uint64_t nlist,
                       const uint64_t *offsets /* host */, const uint64_t *d_ids /* home device */, vidc_shards **out);
/* d_offsets: device uint64[nlist + 1] on the home device; the plan is made on the host, so the offsets cross PCIe once (D2H, as
 * vidc_roc_encode_dev); ntotal must equal d_offsets[nlist]. */
int vidc_shards_encode_dev(vidc_ctx *home, int nshards, vidc_ctx *const *shard_ctxs, int kind, int param, uint32_t flags, uint64_t nlist,
                           const uint64_t *d_offsets, uint64_t ntotal, const uint64_t *d_ids, vidc_shards **out);
void vidc_shards_destroy(vidc_shards *s);
/* host-side accessors: no device work */
int vidc_shards_count(const vidc_shards *s);
int vidc_shards_kind(const vidc_shards *s); /* -1 for NULL */
uint64_t vidc_shards_nlist(const vidc_shards *s);
uint64_t vidc_shards_ntotal(const vidc_shards *s);
/* the sum of the shards' own = the unsharded object's (Elias-Fano: the shards' stream bits are summed before the division by 8) */
uint64_t vidc_shards_compressed_bytes(const vidc_shards *s);
int vidc_shards_map(const vidc_shards *s, int32_t *owner, uint32_t *local_no); /* nlist entries each; either may be NULL */
int vidc_shards_offsets(const vidc_shards *s, uint64_t *offsets);             /* the caller's offsets[nlist + 1] */
/* borrowed: shard i's vidc_packed / vidc_ef / vidc_roc object, for parity tests and for saving shards one by one with the export calls
 * (NULL for a shard without lists); and the context it was built through */
const void *vidc_shards_shard(const vidc_shards *s, int i);
vidc_ctx *vidc_shards_shard_ctx(const vidc_shards *s, int i);
/* Requests: called on the home context the object was built with.  With U = the object vidc_*_encode builds from the same arguments:
 * decode_all = U's decode_all, element for element (the shards decode concurrently, then the inverse cut runs).
 * decode_lists = U's (request order and repeats kept, empty lists allowed; m == 0: VIDC_OK; a list >= nlist: VIDC_ERR_INVALID before any
 *   device work); routed on the host, every involved shard decodes into staging, the copy kernel puts the lists in request order.
 * translate_labels_dev = U's outputs and invalid count (negative labels, lists >= nlist, offsets >= the list's size as there; d_ids ==
 *   d_labels allowed; n == 0 launches nothing; n < 2^32).  A route kernel writes for EVERY shard a full-length local label array
 *   (local_no << 32 | offset where the shard owns the list, -1 elsewhere: nshards * n label slots, no count read-back), each shard's
 *   own translate runs on it, a join kernel picks the owner's answer and adds up the invalid counts.  Unlike the single-object calls this
 *   one WAITS for its join, for every kind; an enqueue-only form is out of scope.
 * decode_gather = U's, signature and checks of vidc_*_decode_gather; items are routed on the host, each involved shard runs its own
 *   decode_gather, a host scatter fills ids_out.  The contexts' vidc_ctx_d2h_bytes grow by 8 * n_items in total.
 * perm = U's permutation in global CSR order (ROC / Elias-Fano built with the perm flag; VIDC_ERR_INVALID otherwise). */
int vidc_shards_decode_all(vidc_ctx *home, const vidc_shards *s, uint64_t *d_out);
int vidc_shards_decode_lists(vidc_ctx *home, const vidc_shards *s, uint64_t m, const uint64_t *list_nos, uint64_t *d_out,
                             uint64_t *out_offsets);
int vidc_shards_translate_labels_dev(vidc_ctx *home, const vidc_shards *s, uint64_t n, const int64_t *d_labels, int64_t *d_ids,
                                     uint64_t *d_invalid);
int vidc_shards_decode_gather(vidc_ctx *home, const vidc_shards *s, uint64_t m, const uint64_t *list_nos, uint64_t n_items,
                              const uint64_t *item_slot, const uint64_t *item_off, int64_t *ids_out);
int vidc_shards_perm(vidc_ctx *home, const vidc_shards *s, uint32_t *perm_host);
/* Append to a sharded object: the "append" section's contract, carried over the shards.  Called on the home context; d_list_nos, d_ids,
 * d_labels (may be NULL) and d_invalid (may be NULL; the caller zeroes it) live on the home device; n_add < 2^32 - 1.
 * Immutable.  *out is a NEW sharded object over the same shard contexts and the same home; `s` stays valid and unchanged, and either may be
 *   destroyed first.
 * The map does not change.  Owner and local number of every list in *out are those of `s`: an append keeps the map, so the balance
 *   drifts with the batches.  vidc_sharded_loads (ids per shard = the sum of the owned lists' sizes; a host accessor, no device work) lets a
 *   caller watch the drift and decide when vidc_rebalance_sharded (below) is worth it.
 * The batch is that of the "append" section: pair i = (d_list_nos[i], d_ids[i]) with GLOBAL list numbers, M_l stable in i, a negative list
 *   number skipped and not counted, one >= nlist skipped and counted in *d_invalid.
 * The result.  Shard k of *out is what vidc_*_append_dev returns for shard k of `s` and the pairs routed to it -- word for word what
 *   vidc_{packed,ef,roc}_encode builds from the cut of M's CSR by the map of `s`; vidc_shards_offsets of *out is M's offsets.  With U' = the
 *   single-object append of the same batch to the unsharded U: every request on *out (decode_all, decode_lists, translate_labels_dev,
 *   decode_gather, perm) returns what U' returns, and d_labels (global list number << 32 | offset, -1 for a skipped pair) and the invalid
 *   count equal U''s.
 * Parameters.  Packed: param = bits, 0 keeps the object's one width, a larger width re-packs every shard, an id that does not fit gives
 *   VIDC_ERR_DOMAIN.  ROC: param = precision_mode (the mode the object was built with).  Elias-Fano: param is ignored.  flags are the
 *   codec's own perm flags and become those of *out.
 * Shards without pairs.  A shard that owns no list holds no object afterwards either.  A shard that holds an object but receives no pair
 *   gets an object equal to its old one (the single-object "batch without a valid pair" case); n_add == 0 returns an equal object.
 * What runs where.  A route kernel on the home stream takes every pair's owner from the device map and writes for EVERY shard a
 *   full-length local list-number array (local_no where the shard owns the list, -1 elsewhere, which the shard's own append skips
 *   uncounted: nshards * n_add slots, batch order and with it the stability contract kept, no count read-back) and an owner byte per pair.
 *   The host waits for the route; then one host thread per shard that holds an object runs the shard's own vidc_*_append_dev, for every
 *   kind.  A shard on the home device reads the caller's d_ids and its slice of the route block in place and writes its labels into the
 *   home block; a shard on another device gets list numbers and ids through hipMemcpyAsync(hipMemcpyDefault) into a staging block of its
 *   own cache, and its labels back -- a path that CANNOT RUN ON A ONE-GPU MACHINE AND HAS NOT BEEN RUN.  A join kernel writes d_labels[i] =
 *   d_list_nos[i] << 32 | the offset of the owner's label.  The new object's offsets are the new shard objects' own list sizes (their
 *   host-side metadata accessors) scattered through the map: O(nlist) host work, as in vidc_shards_encode_dev, and no batch histogram on
 *   the host.  The call WAITS.  vidc_ctx_last_kernel_ms of the home context = route + join.
 * Status.  NULL home / s / out, a NULL array with n_add > 0, n_add >= 2^32 - 1, or a home that is not the object's: VIDC_ERR_INVALID
 *   before any device work.  A status from a shard is returned, "shard i: " in front of its message.  A shard's own invalid count stays 0
 *   (every local number it sees is valid or negative); a non-zero one is an internal error, VIDC_ERR_INVALID.  On any error *out == NULL,
 *   every new shard object already built is destroyed, `s` is untouched and every context stays usable (*d_invalid may have been added to).
 * Residency.  No id payload crosses PCIe: vidc_ctx_d2h_bytes of the home context and of every shard context does not move. */
int vidc_sharded_append_dev(vidc_ctx *home, const vidc_shards *s, uint64_t n_add, const int64_t *d_list_nos, const uint64_t *d_ids,
                            int param, uint32_t flags, vidc_shards **out, int64_t *d_labels, uint64_t *d_invalid);
int vidc_sharded_loads(const vidc_shards *s, uint64_t *loads /* nshards entries: ids per shard */);
/* Remove from a sharded object: the "remove" section's contract, carried over the shards.  Called on the home context; d_list_nos (NULL:
 * any-list mode), d_ids, d_removed (uint8[ntotal_old], may be NULL), d_missing and d_invalid (may be NULL; the caller zeroes them) live on
 * the home device; n_rm < 2^32 - 1.
 * Immutable.  *out is a NEW sharded object over the same shard contexts and the same home; `s` stays valid and unchanged, and either may be
 *   destroyed first.
 * The map does not change.  Owner and local number of every list in *out are those of `s`: a remove keeps the map as an append does.
 *   vidc_sharded_loads of *out shows the drift (vidc_rebalance_sharded undoes it); vidc_shards_offsets of *out is the surviving lists'
 *   offsets.
 * The batch is that of the "remove" section, with GLOBAL list numbers: a negative list number is skipped and not counted, one >= nlist is
 *   skipped and counted in *d_invalid, equality is over all 64 bits, every copy inside a list goes.
 * The result.  With U = the unsharded object of the same lists and (U', mask, missing, invalid) the single-object remove of the same batch
 *   from U: every request on *out (decode_all, decode_lists, translate_labels_dev, decode_gather, perm) returns what U' returns; d_removed
 *   (global decode_all order, every byte written) equals the mask; *d_missing and *d_invalid receive exactly U's increments -- in any-list
 *   mode an id is missing only if NO shard holds it, which is not the sum of the shards' own counts.
 * Shards.  Shard k of *out is, word for word, what vidc_{packed,ef,roc}_encode builds from the cut of the surviving CSR by the map of `s`.
 *   A shard that owns no list holds no object afterwards either; a shard whose lists all become empty holds an ordinary object; the
 *   whole object may become empty.  n_rm == 0, or a batch that matches nothing, returns an equal object and an all-zero mask.
 * Parameters.  Packed: param is ignored, the width stays.  ROC: param = precision_mode (the mode the object was built with).  Elias-Fano:
 *   param is ignored.  flags are the codec's own perm flags and become those of *out.
 * What runs where.  Pairs mode routes as the append does (local_no where a shard owns the list, -1 elsewhere, an owner byte, the invalid
 *   count); any-list mode routes nothing: every shard that holds an object gets NULL list numbers and the caller's d_ids.  The host waits
 *   for the home stream; then one host thread per shard that holds an object runs the shard's own remove, which also answers one FOUND
 *   byte per pair in batch order (1 iff the pair was valid for that shard and its id hit an entry) and the shard's removed mask in its
 *   own decode_all order.  A shard on the home device reads d_ids and its slice of the route block in place and writes mask and found
 *   bytes into the home block; a shard on another device gets list numbers and ids through hipMemcpyAsync(hipMemcpyDefault) into a
 *   staging block of its own cache, and its mask and found bytes back -- a path that CANNOT RUN ON A ONE-GPU MACHINE AND HAS NOT BEEN RUN.
 *   On the home stream the inverse cut on bytes (the OLD plan's segment and chunk tables, a wavefront per 1024 bytes of a segment, 16-byte
 *   accesses where source and destination share their alignment mod 16) writes d_removed, and a join kernel adds to *d_missing the valid
 *   pairs (any-list mode: every pair; pairs mode: those with an owner) whose found byte no shard set.  d_removed == NULL skips the masks
 *   and the inverse cut, d_missing == NULL the found bytes and the join.  The new object's offsets are the new shard objects' own list
 *   sizes scattered through the map, as in the append.  The call WAITS.  vidc_ctx_last_kernel_ms of the home context = route + mask
 *   inverse cut + join.
 * Status.  NULL home / s / out, NULL d_ids with n_rm > 0, n_rm >= 2^32 - 1 (these three before the object is looked into), or a home that
 *   is not the object's: VIDC_ERR_INVALID before any device work.  A status from a shard (a bad precision_mode, say) is returned, "shard
 *   i: " in front of its message.  A shard's own invalid count stays 0; a non-zero one is an internal error, VIDC_ERR_INVALID.  On any
 *   error *out == NULL, every new shard object already built is destroyed, `s` is untouched and every context stays usable (the
 *   counters may have been added to).
 * Residency.  No id payload crosses PCIe: vidc_ctx_d2h_bytes of the home context and of every shard context does not move. */
int vidc_remove_sharded_dev(vidc_ctx *home, const vidc_shards *s, uint64_t n_rm, const int64_t *d_list_nos /* NULL: any-list mode */,
                            const uint64_t *d_ids, int param, uint32_t flags, vidc_shards **out, uint8_t *d_removed, uint64_t *d_missing,
                            uint64_t *d_invalid);
/* Re-balance a sharded object: the lists of `s` under the map vidc_shards_encode_dev would choose for what `s` decodes to -- the
 * longest-processing-time rule on vidc_shards_offsets(s).  Called on the home context.
 * Immutable.  *out is a NEW sharded object over the same shard contexts and the same home; `s` stays valid and unchanged, and either may be
 *   destroyed first.  One shard, or a map that does not change, returns an equal object.
 * The result.  decode_all, decode_lists, translate_labels_dev and decode_gather answer on *out exactly as on `s` (ROC's sampling order
 *   included); vidc_shards_offsets, ntotal and compressed_bytes are those of `s`; vidc_shards_map and vidc_sharded_loads are the new
 *   map's.  flags are the codec's own perm flags and become those of *out: with the perm flag vidc_shards_perm of *out is the identity
 *   inside every list (a permutation of a derived object is over the positions of what the old lists decode to).
 *   *moved_ids (host, may be NULL) = the number of ids whose owner changed, host arithmetic on the two maps.
 * Shards.  A shard that owns no list under the new map holds no object.  Packed bits (the object's width is kept), Elias-Fano: shard k of
 *   *out is, word for word, what vidc_{packed,ef}_encode builds from the new map's cut of decode_all(s).  ROC: for every global list the
 *   new owner's list equals the old owner's list in size, precision, head, nwords, mt_draws and every word.  For the lists the encoder
 *   reproduces -- distinct ids, at most 65 536 of them, no power-of-two maximum under VIDC_PREC_REFERENCE -- that is also, word for word,
 *   what vidc_roc_encode builds from the new cut with the object's param; any other list keeps its old stream, as an untouched list does
 *   in an append.
 * What runs where.  Packed bits and Elias-Fano are REBUILT: vidc_shards_decode_all into a block of the home cache, then the body of
 *   vidc_shards_encode_dev on the object's own offsets; no id reaches the host.  ROC lists MOVE AS STREAMS: the host makes, per new shard,
 *   one (old shard, old local number) row per local list; one host thread per new shard that owns lists calls vidc_roc_regroup on its
 *   context with the old shard objects as sources -- no ANS chain runs, and a shard that already has its final content still gets a
 *   regrouped object of its own.  An old shard on another device than its destination first regroups the lists bound there into a
 *   temporary object on its own context; the destination copies that object's arrays into its own cache with
 *   hipMemcpyAsync(hipMemcpyDefault) and regroups from the copy -- a path that CANNOT RUN ON A ONE-GPU MACHINE AND HAS NOT BEEN RUN.  The
 *   call WAITS.
 * Status.  NULL home / s / out, or a home that is not the object's: VIDC_ERR_INVALID before any device work.  A status from a shard is
 *   returned, "shard i: " in front of its message.  On any error *out == NULL, every new shard object already built is destroyed, `s`
 *   is untouched and every context stays usable.
 * Residency.  No id payload crosses PCIe: vidc_ctx_d2h_bytes of no context moves (ROC reads back one 8-byte word total per regroup,
 *   metadata, which that counter does not count). */
int vidc_rebalance_sharded(vidc_ctx *home, const vidc_shards *s, uint32_t flags, vidc_shards **out, uint64_t *moved_ids /* host, may be NULL */);

/* ------------------------------------------------ segmented ROC lists (parallel chains inside a list) */
/* A ROC list is one chain of dependent ANS steps; a list of 50 000 ids is a chain of 50 000.  A set of ids cut BY VALUE RANGE into
 * segments costs the same number of bits up to a constant per segment, and every segment is an independent chain over a smaller
 * universe.  vidc_rocseg is the opt-in container built on that: like VIDC_PREC_EXACT it is NOT reference-identical (the reference has one
 * stream per list); nothing about vidc_roc changes.
 *
 * Parameters.  seg_ids = T, a power of two in [16, 65 536] (0: VIDC_ROCSEG_DEFAULT_IDS): the target number of ids per segment.
 *   universe_bits = B in 1 .. 31 (0: max(1, bit_width(largest id of the call)), found by a reduction on the device).  An id >= 2^B is
 *   VIDC_ERR_DOMAIN.  The per-list domain is that of vidc_roc_encode.
 * Segments.  List l with n_l ids has S_l = 2^k_l segments, k_l = 0 for n_l <= T and min(B, ceil_log2(ceil(n_l / T))) otherwise, and
 *   shift_l = B - k_l: id x sits in segment x >> shift_l and is stored as x & (2^shift_l - 1) (k_l = 0: one segment, the id unchanged).
 *   S_l > VIDC_ROCSEG_MAX_SEGS is VIDC_ERR_DOMAIN.  A segment keeps its ids in the input order of its list: the partition is stable,
 *   and no atomic decides a position.
 * The inner object is an ordinary vidc_roc over the sum of S_l lists in (list, segment) order, encoded with VIDC_PREC_EXACT (rebasing
 *   makes power-of-two maxima all the time, which the reference precision loses): every segment is, word for word, what vidc_roc_encode
 *   builds from its rebased ids at bit_width(max); empty segments are empty lists.  Segments of a list are consecutive, so the inner CSR
 *   addresses the same positions as the outer one and decode_all decodes straight into the caller's buffer.
 * Order.  A list decodes as its segments in order, each in its own sampling order.  vidc_rocseg_perm maps output position to input
 *   position within the list, as vidc_roc_perm does (objects encoded with VIDC_ROC_WANT_PERM; VIDC_ERR_INVALID otherwise).
 * Size.  compressed_bytes = the inner object's + 4 bytes for every segment of a list with S_l > 1.
 * Requests answer as the vidc_roc calls of the same name do: decode_lists expands the outer list numbers into inner ranges on the host
 *   and collapses out_offsets back to m + 1; translate_labels_dev rewrites the labels on the device (a binary search over the list's
 *   inner offsets; a negative label stays negative, an invalid one is counted once), runs vidc_roc_translate_labels_dev on them -- only
 *   the TOUCHED SEGMENTS decode -- and adds the segment bases to the results >= 0; d_ids == d_labels is allowed.  Behind every decode a
 *   wavefront per 1024-id chunk ORs segment << shift into the decoded ids in place.  The calls wait; vidc_ctx_last_kernel_ms is the sum
 *   of the inner call's kernels and the container's own, and vidc_ctx_phase_ms(VIDC_PHASE_ROCSEG_PARTITION) the encode's own kernels.
 * vidc_rocseg_inner is borrowed: the vidc_roc list_info / export calls on it serve parity checks and saving.  vidc_rocseg_seg_info copies
 *   the map: seg_first[l] = the first inner list of list l (nlist + 1 entries), shift[l] (nlist entries); either may be NULL.
 * vidc_rocseg_wrap builds a segmented object from an imported inner object (vidc_roc_import) and an UNTRUSTED map; on success it takes
 *   ownership of `inner`.  Checked before any device work: seg_first monotone from 0 to the inner object's list count, every segment count
 *   a power of two <= VIDC_ROCSEG_MAX_SEGS that equals 2^(universe_bits - shift), every inner precision <= its list's shift (a decoded id
 *   then stays below its segment's width), seg_ids and universe_bits in range (no 0 defaults here).  Anything else: VIDC_ERR_INVALID,
 *   *out == NULL, and `inner` stays the caller's.  A wrapped object carries no permutation.
 * Status.  NULL arguments, a seg_ids that is not a power of two in range, universe_bits > 31: VIDC_ERR_INVALID before any device work.  On
 *   any error *out == NULL and the context stays usable.
 * Out of scope: append, remove, regroup, sharding and graph rows on segmented objects (re-encode, or use vidc_roc). */
typedef struct vidc_rocseg vidc_rocseg;
#define VIDC_ROCSEG_MAX_SEGS 1024u
#define VIDC_ROCSEG_DEFAULT_IDS 1024u /* the fastest of 1024 .. 8192 on S1 and on 16.8 M ids / 65 536 Zipf lists: DESIGN 9c, profiles/r33_roc_segmented.json */
int vidc_rocseg_encode(vidc_ctx *ctx, uint64_t nlist, const uint64_t *offsets /* host */, const uint64_t *d_ids, uint32_t seg_ids,
                       uint32_t universe_bits, uint32_t flags /* VIDC_ROC_WANT_PERM */, vidc_rocseg **out);
/* d_offsets: device uint64[nlist + 1]; the plan is made on the host, so the offsets cross PCIe once (as vidc_roc_encode_dev) */
int vidc_rocseg_encode_dev(vidc_ctx *ctx, uint64_t nlist, const uint64_t *d_offsets, uint64_t ntotal, const uint64_t *d_ids, uint32_t seg_ids,
                           uint32_t universe_bits, uint32_t flags, vidc_rocseg **out);
void vidc_rocseg_destroy(vidc_rocseg *s);
uint64_t vidc_rocseg_nlist(const vidc_rocseg *s);
uint64_t vidc_rocseg_ntotal(const vidc_rocseg *s);
uint64_t vidc_rocseg_compressed_bytes(const vidc_rocseg *s);
uint32_t vidc_rocseg_seg_ids(const vidc_rocseg *s);
uint32_t vidc_rocseg_universe_bits(const vidc_rocseg *s);
const vidc_roc *vidc_rocseg_inner(const vidc_rocseg *s);
int vidc_rocseg_seg_info(const vidc_rocseg *s, uint64_t *seg_first /* nlist + 1 */, uint8_t *shift /* nlist */);
int vidc_rocseg_wrap(vidc_ctx *ctx, vidc_roc *inner, uint64_t nlist, const uint64_t *seg_first, const uint8_t *shift, uint32_t seg_ids,
                     uint32_t universe_bits, vidc_rocseg **out);
int vidc_rocseg_decode_all(vidc_ctx *ctx, const vidc_rocseg *s, uint64_t *d_out);
int vidc_rocseg_decode_lists(vidc_ctx *ctx, const vidc_rocseg *s, uint64_t m, const uint64_t *list_nos, uint64_t *d_out,
                             uint64_t *out_offsets);
int vidc_rocseg_translate_labels_dev(vidc_ctx *ctx, const vidc_rocseg *s, uint64_t n, const int64_t *d_labels, int64_t *d_ids,
                                     uint64_t *d_invalid);
int vidc_rocseg_perm(vidc_ctx *ctx, const vidc_rocseg *s, uint32_t *perm_host);
/* vidc_roc_last_decode_handed_back of the inner object */
uint64_t vidc_rocseg_last_decode_handed_back(const vidc_rocseg *s);

/* ------------------------------------------------------ introspection / timing */
/* Milliseconds spent inside the kernels of the most recent encode / decode call on this context,
 * measured with hipEvents on the context's stream (used by bench.py for the roofline figure). */
double vidc_ctx_last_kernel_ms(const vidc_ctx *ctx);
/* Per-phase kernel time (ms, hipEvents) of the most recent call that ran the phase. */
#define VIDC_PHASE_ROC_ENCODE 0  /* k_roc_encode_tiny + k_roc_encode_gen launches */
#define VIDC_PHASE_ROC_COMPACT 1 /* k_roc_compact */
#define VIDC_PHASE_ROC_DECODE 2  /* k_roc_decode_gen + k_roc_decode_tiny launches */
#define VIDC_PHASE_ROC_ENCODE_CHAIN 3 /* the ONE launch holding the call's longest chains (k_roc_encode_u2<20/18>): its duration */
#define VIDC_PHASE_ROC_DECODE_CHAIN 4 /* k_roc_decode_u2<20/18>, same */
#define VIDC_PHASE_IMPORT_H2D 5 /* vidc_wt_import / vidc_compact_import: the host -> device copies of the image.  The kernels that rebuild
                                 * and check are vidc_ctx_last_kernel_ms: for wt_type 1 the sum of the intervals in front of and behind the
                                 * read-back of the levels' width totals, without the wait between them */
#define VIDC_PHASE_ROC_REGROUP_COPY 6 /* vidc_roc_regroup: the segmented word copy alone (0 for an object without words) */
#define VIDC_PHASE_ROCSEG_PARTITION 7 /* vidc_rocseg_encode*: the universe reduction, the multisplit, its scan, the inner offsets and the
                                       * permutation compose -- everything but the inner vidc_roc_encode_dev */
#define VIDC_PHASE_COUNT 8
double vidc_ctx_phase_ms(const vidc_ctx *ctx, int phase);
/* What the chain launch of the last ROC encode (which = 0) / decode (1) on this context processed: ids, lists, longest list and
 * the universe (18 or 20 bits; 0 when the call had no such class).  bench.py derives the dominant kernel's roofline from it. */
int vidc_ctx_chain_info(const vidc_ctx *ctx, int which, uint64_t *ids, uint64_t *lists, uint64_t *longest, uint32_t *universe_bits);

#ifdef __cplusplus
}
#endif
#endif
