/*
 * vssgpu.h — C ABI of the MI355X-native HNSW / array-distance engine (libvssgpu.so).
 *
 * This is the drop-in boundary for the one member the reference's HNSWIndex delegates all of its arithmetic
 * to: `unum::usearch::index_dense_gt<row_t> index` (reference src/include/hnsw/hnsw_index.hpp:45).  Every entry
 * point below names the reference call it replaces.  Plain C: pointers + sizes, int status codes, no
 * exceptions and no torch / HIP types in the signatures (a hipStream_t travels as void*).
 *
 * Status convention: 0 = VSS_OK, anything else = failure with a message in vss_last_error()
 * (mirrors `result.error.what()` of usearch's result structs — reference hnsw_index.cpp:474-476,
 * hnsw_index_physical_create.cpp:188-193).
 *
 * Pointer convention: functions ending in `_device` take DEVICE pointers (already resident in HBM) and are
 * asynchronous on the index's stream; all others take HOST pointers, copy, and return when results are valid.
 *
 * Threading: one handle may be used from any number of host threads.  Searches, exact searches, statistics, vss_timing and
 * vss_save run concurrently (reader lock; each blocking call leases one of eight internal search contexts — the analogue of the
 * usearch context a thread leases, index_dense.hpp:1730-1745); calls that change the index (stage, finalize, add, remove,
 * compact, load, reserve, set_*) are exclusive, as under DuckDB's index lock (hnsw_index.cpp:388, 421, 496).  The explicit
 * contexts 0..3 of vss_search_*_begin / vss_search_batch_end belong to the caller; a mutating call made while one of
 * them has a probe in flight is refused.  vss_last_error() is per calling thread.
 */
#ifndef VSSGPU_H
#define VSSGPU_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct vss_index vss_index;

enum { VSS_OK = 0, VSS_ERROR = 1 };

/* Index metric — reference hnsw_index.cpp:264-268 (METRIC_KIND_MAP: "l2sq" | "cosine" | "ip").
 * Distances are usearch's: l2sq = sum (a-b)^2 (no sqrt), cosine = 1 - cos, ip = 1 - a.b
 * (index_plugins.hpp:977-1053). */
enum { VSS_METRIC_L2SQ = 0, VSS_METRIC_COSINE = 1, VSS_METRIC_IP = 2 };

/* SQL scalar functions over FLOAT[N] — named at reference hnsw_index.cpp:659-673 (DuckDB core v1.4.3):
 * array_distance = sqrt(sum (a-b)^2), array_cosine_distance = 1 - cos, array_negative_inner_product = -a.b */
enum { VSS_FN_ARRAY_DISTANCE = 0, VSS_FN_ARRAY_COSINE_DISTANCE = 1, VSS_FN_ARRAY_NEGATIVE_INNER_PRODUCT = 2 };

/* Tombstone key: std::numeric_limits<row_t>::max() — usearch index.hpp:990, index_dense.hpp:435. */
#define VSS_FREE_KEY INT64_MAX

/* ---- lifetime ------------------------------------------------------------------------------------------- */

/* Replaces index_dense_gt<row_t>::make(metric_punned_t(dim, kind, f32), config) with
 * config.{connectivity=M, connectivity_base=M0, expansion_add=ef_construction, expansion_search=ef_search}
 * — reference hnsw_index.cpp:190-219.  `device` is the HIP device ordinal the index lives on.  M0 < M is refused (the
 * reference overruns its base lists there). */
int vss_create(uint64_t dim, int metric, uint64_t M, uint64_t M0, uint64_t ef_construction, uint64_t ef_search,
               int device, vss_index **out);
/* index.reset() / destructor — reference hnsw_index.cpp:414. */
void vss_destroy(vss_index *index);
/* result.error.what() of the calling thread's last failed call on any handle; valid until its next call. */
const char *vss_last_error(vss_index *index);
/* Run the index's kernels on a caller-owned hipStream_t (NULL = the engine's own stream). */
int vss_set_stream(vss_index *index, void *hip_stream);
/* Block until everything queued on the index's stream has finished. */
int vss_synchronize(vss_index *index);

/* ---- build ---------------------------------------------------------------------------------------------- */

/* index.reserve({members, threads}) — reference hnsw_index_physical_create.cpp:300, hnsw_index.cpp:238,459.
 * Grows device storage; a growing reserve restarts the level generator exactly like usearch replaces its
 * thread contexts (index.hpp:2485,2496). */
int vss_reserve(vss_index *index, uint64_t members, uint64_t threads);

/* Bulk path, step 1 (replaces the Sink/Combine materialisation + the per-row loop of
 * HNSWIndexConstructTask::ExecuteTask, reference hnsw_index_physical_create.cpp:102-110,148-209): copy a
 * chunk of `count` rows (vecs = count x dim contiguous floats, the ARRAY child vector; rowids = row_t[count];
 * validity = DuckDB validity mask words or NULL, a cleared bit means NULL row: skipped exactly like
 * hnsw_index.cpp:467-470) into device storage, draw each row's level, leave it unlinked. */
int vss_stage_batch(vss_index *index, const int64_t *rowids, const float *vecs, const uint64_t *validity,
                    uint64_t count);
int vss_stage_batch_device(vss_index *index, const int64_t *d_rowids, const float *d_vecs, uint64_t count);
/* Bulk path, step 2 (replaces the N concurrent index.add streams scheduled by
 * HNSWIndexConstructionEvent::Schedule, reference hnsw_index_physical_create.cpp:235-247): link every staged
 * row into the graph with the batch-synchronous GPU build. */
int vss_build_finalize(vss_index *index);
/* Incremental path: index.add(rowid, vec) for every valid row of a chunk — reference HNSWIndex::Construct,
 * hnsw_index.cpp:463-478.  Equivalent to vss_stage_batch + vss_build_finalize.  Capacity must have been
 * reserved ("Reserve capacity ahead of insertions!" otherwise, as usearch index.hpp:2728-2731). */
int vss_add_batch(vss_index *index, const int64_t *rowids, const float *vecs, const uint64_t *validity,
                  uint64_t count);
/* Tuning of the batch-synchronous build: batch = clamp(nodes / growth_div, 1, max_batch).  No reference counterpart
 * (usearch's parallel build — N add() streams, hnsw_index_physical_create.cpp:235-247 — has no schedule); with
 * max_batch = 1 the build is the reference's sequential add() loop. */
int vss_set_build_params(vss_index *index, uint64_t max_batch, uint64_t growth_div);
/* on != 0: a bulk build into an EMPTY index (vss_build_finalize after staging from scratch) ends with the reordering of
 * vss_compact — the reference's own compaction order, index_gt::compact index.hpp:3405-3494 — so that a freshly built index
 * already has the nodes of a cluster contiguous in HBM.  Off by default (the reference does not reorder on CREATE INDEX
 * either); costs one greedy descent per node (about 1 s per 10M x 768 rows) and changes no answer except the order of rows
 * at exactly equal distance. */
int vss_set_build_reorder(vss_index *index, int on);

/* ---- search --------------------------------------------------------------------------------------------- */

/* Tuning options of the search engine — NO reference counterpart, and NOTHING a DuckDB integration has to call: every option
 * has a default that is the measured best, and results (row ids, distances, counts, work counters) never depend on any of them.
 * They exist for A/B measurements and for the tests that force every engine shape.  (Rounds 2-5 exported one setter per knob;
 * round 6 folded them into this one call — the ABI a maintainer reads is the reference's call sites, not the builder's
 * switches.)  `name`:
 *   search.waves (2..16) / search.walkers (0 = per launch ..8)   wavefronts per workgroup, and how many of them walk a query
 *   search.solo (0 never, 1 automatic, 2 always) / search.solo_max_queries   one single-wave workgroup per query (few queries, narrow rows)
 *   search.team (0/1)            eight-wave teams in the solo shape
 *   search.crew (0/1; 1|16|4|8 = refinements)   the last walker of a workgroup runs its scoring waves behind barriers
 *   search.pipelined (0/1)       accept phase in the shadow of the successor's row loads (exact)
 *   search.wide_lists (0/1)      limits of 257-512 in 12-wave workgroups
 *   search.visited_compact (0/1) / search.visited_lds_log2_max (0 = default, <= 14) / search.visited_cells_per_limit (0 = rule, >= 4)
 *                                / search.retry_in_place (0/1)     where a walker's visited set lives and what happens when it overflows
 *   search.probe_flag_wait (0/1) host-pointer probes of <= 256 queries wait on a pinned flag instead of the stream
 *   search.lookahead (0..8)      one expansion of look-ahead (off: measured slower)
 *   search.gating (0/1)          a launch is issued when its predecessor on the device starts to drain
 *   search.list_lds (0..2)       candidate lists of limits 513-4096 in LDS: 0 never (HBM), 1 automatic (when the workgroup keeps
 *                                its walkers), 2 whenever one walker fits; vss_last_search_shape reports the placement
 *   search.prescore (0..2)       scoring waves reject rows on exact lower bounds from 8-bit row codes before they read the rows'
 *                                f32 components (rows of 512 / 768 / 1024 / 1536 dimensions, plain batched searches): 0 never (no
 *                                codes held), 1 at limits of at most 256 (default: where it gains), 2 at limits of 257-512 as well;
 *                                costs a quarter of the vectors' bytes again in device memory; vss_last_search_prescore reports it
 *   search.prescore_descent (0/1) in the launches that filter on row codes, the greedy descent's rows are bounded too, against the
 *                                descent's closest distance (default 1; 0: the descent scores every row it gathers);
 *                                vss_last_search_prescore_descent reports it
 * Unknown names and values out of range are refused (VSS_ERROR, vss_last_error says which); the environment variables of the
 * same knobs (tools/README.md) are read once, in vss_create, through the same checks.  DESIGN.md §4.2 describes each mechanism. */
int vss_set_option(vss_index *index, const char *name, int64_t value);

/* index.ef_search(query, k, ef).dump_to(row_ids) — reference HNSWIndex::InitializeScan hnsw_index.cpp:315-341.
 * ef = 0 means the index's ef_search option.  Writes <= k row ids in ascending distance order, returns the
 * count through *out_count. */
int vss_search(vss_index *index, const float *query, uint64_t k, uint64_t ef, int64_t *out_rowids,
               uint64_t *out_count);
/* The batched probe of PhysicalHNSWIndexJoin::Execute (reference hnsw_optimize_join.cpp:111-168): n_queries
 * independent ef_search calls (hnsw_index.cpp:383-397) issued as ONE kernel launch.  queries = n_queries x dim.
 * out_rowids = n_queries x k (unused tail cells = -1), out_distances optional (index metric, may be NULL),
 * out_counts = results per query. */
int vss_search_batch(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                     int64_t *out_rowids, float *out_distances, uint32_t *out_counts);
int vss_search_batch_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                            int64_t *d_out_rowids, float *d_out_distances, uint32_t *d_out_counts);
/* index.filtered_search(query, k, predicate) — usearch index_dense.hpp:625-629 with expansion = ef: a row is admitted to
 * the result iff it is live AND bit `rowid` of `allowed` is set (rows with rowid >= n_bits are rejected); rejected rows
 * are still traversed, exactly like tombstones (index.hpp:3986-3992).  This pushes a WHERE predicate INTO the traversal
 * instead of filtering above the scan as the reference does (hnsw_optimize_scan.cpp:168-198, which can return fewer than
 * k rows) — SURVEY §8f rank 3.  `allowed` = (n_bits + 63) / 64 words. */
int vss_search_batch_filtered(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                              const uint64_t *allowed, uint64_t n_bits, int64_t *out_rowids, float *out_distances,
                              uint32_t *out_counts);
int vss_search_batch_filtered_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                     const uint64_t *d_allowed, uint64_t n_bits, int64_t *d_out_rowids,
                                     float *d_out_distances, uint32_t *d_out_counts);
/* The same with ONE PREDICATE PER QUERY, in one launch: the chunk of PhysicalHNSWIndexJoin::Execute
 * (hnsw_optimize_join.cpp:111-168) whose LATERAL subquery is correlated — `WHERE items.tenant = q.tenant` — so that every
 * outer row has its own filtered_search predicate (index_dense.hpp:625-629).  `allowed` = n_groups bitmaps laid end to end, each
 * words = (n_bits + 63) / 64 words, group g at allowed + g * words; group_of[q] < n_groups names the bitmap of query q.
 * Query q gets exactly what vss_search_batch_filtered returns for it alone with bitmap allowed + group_of[q] * words and the
 * same n_bits — row ids, distance bits, count; tombstones excluded, rejected rows traversed, row ids >= n_bits rejected (a
 * set padding bit after n_bits admits nothing, whatever group follows it).  There is no "no predicate" group number: pass a
 * group of all ones.  Outputs are laid out as vss_search_batch_filtered's; after the host-pointer form vss_last_search_stats /
 * vss_last_search_query_stats describe the call as they do there.
 * VSS_ERROR: allowed or group_of NULL, or n_groups == 0, with n_queries > 0; no device memory for the table.  Host-pointer
 * form: a group_of[q] >= n_groups is refused before anything is launched (the message names the first such query).  Device
 * form: the engine does not copy group_of back to look; such a query is answered as if its predicate admitted nothing —
 * count 0, cells -1 / +inf — and nothing outside the n_groups * words words is read.
 * The pipelined and multi-batch forms are vss_search_batch_filtered_groups_device_begin and
 * vss_search_multi_filtered_device_begin, below. */
int vss_search_batch_filtered_groups(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                     const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits, const uint32_t *group_of,
                                     int64_t *out_rowids, float *out_distances, uint32_t *out_counts);
int vss_search_batch_filtered_groups_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k,
                                            uint64_t ef, const uint64_t *d_allowed, uint64_t n_groups, uint64_t n_bits,
                                            const uint32_t *d_group_of, int64_t *d_out_rowids, float *d_out_distances,
                                            uint32_t *d_out_counts);
/* Exact top-k under per-query predicates, scanning only the admitted rows: the call for a SELECTIVE predicate (a tenant join),
 * where the graph calls above traverse every rejected row like a tombstone.  Table layout and admission rule are those of
 * vss_search_batch_filtered_groups: n_groups bitmaps of (n_bits + 63) / 64 words end to end, query q filtered by bitmap
 * group_of[q]; a row is admitted iff it is live, 0 <= rowid < n_bits and bit rowid is set (a set padding bit after n_bits
 * admits nothing, whatever group follows it).  group_of == NULL is legal HERE: every query takes bitmap 0.
 * For finite inputs query q gets the min(k, admitted live rows) admitted rows with the smallest (distance, slot) pairs, in
 * that order; `distance` is the engine's f32 metric, the bits vss_search_batch reports for that pair.  Outputs are laid out as
 * vss_search_exact_batch's (unused cells -1 / +inf; out_distances may be NULL).  Distances are the metric's own throughout — no
 * ranking score, no certificate, no fallback: vss_last_exact_fallbacks is 0 after the call, and answers depend on no option.
 * Mechanism (csrc/exact_filtered_kernels.h): for every group that has a query, the ascending list of its live admitted
 * slots; rows are scored through the lists, MS_QT queries of one group per workgroup; the k + 8 best (distance, slot) pairs
 * per query are re-ranked as vss_search_exact_batch re-ranks.  Scratch: the lists of one pass hold at most max(B, rows)
 * entries of 4 bytes, B = 2^23 or VSS_EXACT_FILTER_LIST_ENTRIES (read in vss_create); groups are packed into passes in group
 * order.  The scratch is counted in vss_memory_usage while it is held.
 * k <= 4088.  VSS_ERROR with a message: allowed NULL or n_groups == 0 (with n_queries > 0 and k > 0); a table no size_t can
 * hold; a row that does not fit the scoring kernel's LDS; no device memory.  Host form: a group_of[q] >= n_groups is refused
 * before anything runs (the message names the first such query).  Device form: such a query gets count 0, cells -1 / +inf;
 * the engine copies d_group_of back (4 bytes per query) for its plan.  n_queries == 0 or k == 0: VSS_OK.  An empty index
 * answers count 0 everywhere.  Takes the reader lock and the exact path's mutex, as vss_search_exact_batch does; the device
 * form runs on the index stream and its results are valid when it returns. */
int vss_search_exact_batch_filtered_groups(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k,
                                           const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits,
                                           const uint32_t *group_of, int64_t *out_rowids, float *out_distances,
                                           uint32_t *out_counts);
int vss_search_exact_batch_filtered_groups_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k,
                                                  const uint64_t *d_allowed, uint64_t n_groups, uint64_t n_bits,
                                                  const uint32_t *d_group_of, int64_t *d_out_rowids, float *d_out_distances,
                                                  uint32_t *d_out_counts);
/* The last such call: out4[0] = admitted rows listed, summed over the groups that had queries; [1] = (query, row) distances
 * computed; [2] = passes; [3] = bytes of list scratch held.  Results never depend on it. */
int vss_last_exact_filtered(vss_index *index, uint64_t *out4);
/* Per-query predicates, every GROUP answered by the cheaper of the two calls above — the call for a chunk that names large and
 * tiny tenants at once, and for a caller that has bitmaps but no idea how many live rows each admits.  Table layout, n_bits and
 * the admission rule are those of the two calls; group_of == NULL is legal (every query takes bitmap 0).
 * The rule (csrc/filter_route.h): the engine counts len_u, the live admitted rows of every group u in use, on the device — the
 * first step of the exact call, run once — and group u goes EXACT iff  len_u^2 * 64 <= C * limit * L,  where L = live linked
 * rows, limit = max(k, ef) (ef == 0: the index's ef_search) and C = route_c, or 62 500 where route_c == 0.  len_u == 0 and an
 * empty index are exact; route_c == UINT64_MAX routes everything exact.  route_c is an argument and no option of
 * vss_set_option because it can change an answer.  Under a named route_c a query's route depends on its group alone, never on
 * the other groups or on the batch size.  With route_c == 0 one more step applies, the minimum walk: where some exact-routed
 * group admits a row (so lists are built anyway) and the graph-routed groups together amount to fewer than 2^24
 * (query, admitted row) pairs, those groups are scanned as well — a walk is a launch of its own and has a floor of one to three
 * milliseconds.
 * out_route (may be NULL), one byte per query: 0 = graph, 1 = exact, 255 = its group is not in the table (device form only).
 * Contract: a query of route 1 gets, bit for bit (row ids, f32 distances, count), what vss_search_exact_batch_filtered_groups
 * gives it; a query of route 0 what vss_search_batch_filtered_groups gives it under the same k and ef (group_of == NULL:
 * vss_search_batch_filtered with bitmap 0); a query of route 255 count 0, cells -1 / +inf.  out_distances may be NULL.
 * Mechanism (csrc/filter_route_kernels.h): lists are built for exact-routed groups only and their queries answered straight
 * into the caller's cells; the graph-routed queries are gathered into a compact batch, walked by ONE ordinary filtered search
 * launch — no walker sees an exact-routed query, and there is no launch when nothing is graph-routed — and scattered back.
 * The two parts run one after the other.
 * Errors are those of the two calls; the host form refuses a group_of[q] >= n_groups before anything runs (the message names
 * the first such query); k <= 4088 holds only if some query is exact-routed.  n_queries == 0 or k == 0: VSS_OK.
 * Reader lock; the exact path's mutex around the count and the exact part; the host form walks on a leased context, the
 * device form on the index stream (context 0) and copies d_group_of back (4 bytes per query).  d_out_route is device memory
 * there.  Results are valid when the call returns.
 * Afterwards vss_last_search_stats / _shape / _prescore describe the graph part (all zero if there was none; per-query
 * counters are not kept), vss_last_exact_filtered the exact part ([0] = rows listed over the exact-routed groups in use). */
int vss_search_batch_filtered_groups_auto(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                          const uint64_t *allowed, uint64_t n_groups, uint64_t n_bits, const uint32_t *group_of,
                                          uint64_t route_c, int64_t *out_rowids, float *out_distances, uint32_t *out_counts,
                                          uint8_t *out_route);
int vss_search_batch_filtered_groups_auto_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k,
                                                 uint64_t ef, const uint64_t *d_allowed, uint64_t n_groups, uint64_t n_bits,
                                                 const uint32_t *d_group_of, uint64_t route_c, int64_t *d_out_rowids,
                                                 float *d_out_distances, uint32_t *d_out_counts, uint8_t *d_out_route);
/* The last such call: out8[0] = queries routed graph, [1] = queries routed exact, [2] / [3] = groups in use routed graph /
 * exact, [4] = L, [5] = the C used, [6] = limit, [7] = 0. */
int vss_last_filter_route(vss_index *index, uint64_t *out8);

/* ---- Equality predicates on a resident label column (csrc/label_filter.h) ------------------------------------------------
 * For the predicate `items.tenant = q.tenant`: the index keeps one 32-bit label per ROW ID on the device, a query brings the
 * one value it wants, and no bitmap is built, uploaded or read.  The column is indexed by row id like the bitmaps of the
 * calls above, so removals, reused slots and vss_compact need no label call; it is NOT part of the stream (vss_save) and
 * vss_load clears it — set the labels again after a load.  Every other predicate keeps the bitmap calls.
 *
 * vss_set_labels writes cells first_rowid .. first_rowid + n - 1 (overwriting), grows the column when it must and fills a
 * gap it skips over with VSS_NO_LABEL.  first_rowid + n > 2^32 is refused; n == 0 is a no-op.  Without room on the device
 * the call fails and the column stays as it was.  Writer lock; refused while a _begin context is in flight.
 * vss_labelled_rows: row ids [0, this) have a cell; 0 = no column.  vss_memory_usage counts the column. */
#define VSS_NO_LABEL 0xFFFFFFFFu
int vss_set_labels(vss_index *index, uint64_t first_rowid, const uint32_t *labels, uint64_t n); /* host memory */
int vss_set_labels_device(vss_index *index, uint64_t first_rowid, const uint32_t *d_labels, uint64_t n);
int vss_clear_labels(vss_index *index);
uint64_t vss_labelled_rows(const vss_index *index);
/* Query q admits a live row of id r iff 0 <= r < vss_labelled_rows(), labels[r] == want[q] and want[q] != VSS_NO_LABEL (a
 * NULL tenant equals nothing: count 0, ids -1, distances +inf — as for a value no row carries).
 * mode: VSS_BY_LABEL_GRAPH the walk of vss_search_batch_filtered_groups, VSS_BY_LABEL_EXACT the scan of
 * vss_search_exact_batch_filtered_groups (ef unused), VSS_BY_LABEL_AUTO the rule and minimum walk of ..._groups_auto with
 * the same route_c.  out_route (may be NULL): all 0 in mode GRAPH, all 1 in mode EXACT, the routes in mode AUTO.
 * Contract: with v_0 < v_1 < ... the distinct values of `want`, bitmap g = {r < labelled rows : labels[r] == v_g != VSS_NO_LABEL}
 * and group_of[q] = the index of want[q], the call returns cell for cell what the bitmap call of the same mode returns for
 * that table — row ids, f32 distance bits, counts, routes — and leaves the same vss_last_exact_filtered [0..2],
 * vss_last_filter_route, vss_last_search_stats / _shape / _prescore values behind.
 * Errors: no column set; a mode other than the three (refused before anything is staged); those of the call of the mode.
 * The _device form takes device pointers (d_out_distances and d_out_route may be NULL), copies d_want back (4 bytes per
 * query) and runs on context 0.  The pipelined / multi-batch forms: vss_search_by_label_device_begin, below. */
enum { VSS_BY_LABEL_GRAPH = 0, VSS_BY_LABEL_EXACT = 1, VSS_BY_LABEL_AUTO = 2 };
int vss_search_batch_by_label(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                              const uint32_t *want, int mode, uint64_t route_c, int64_t *out_rowids, float *out_distances,
                              uint32_t *out_counts, uint8_t *out_route);
int vss_search_batch_by_label_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                     const uint32_t *d_want, int mode, uint64_t route_c, int64_t *d_out_rowids,
                                     float *d_out_distances, uint32_t *d_out_counts, uint8_t *d_out_route);
/* ---- Range predicates on the same column (csrc/label_filter.h) -----------------------------------------------------------
 * For `items.ts >= q.since`, `items.price BETWEEN q.lo AND q.hi`, `items.day < q.cutoff`: query q brings an inclusive range
 * [lo[q], hi[q]] of UNSIGNED 32-bit labels (INTEGRATION.md section 5 has the order-preserving maps from INTEGER, FLOAT and DATE).
 * Query q admits a live row of id r iff 0 <= r < vss_labelled_rows(), labels[r] != VSS_NO_LABEL and lo[q] <= labels[r] <= hi[q].
 * lo[q] > hi[q] is the empty predicate (count 0, ids -1, distances +inf); hi[q] = 0xFFFFFFFF is "no upper bound", and a cell
 * holding VSS_NO_LABEL is admitted by no range.  mode, route_c and out_route as for vss_search_batch_by_label.
 * Contract: with p_0 < p_1 < ... the distinct RAW pairs (lo, hi) of the call, ascending lexicographically and not canonicalised
 * (two different empty pairs are two groups), bitmap g = {r < labelled rows : labels[r] != VSS_NO_LABEL and labels[r] in p_g}
 * and group_of[q] = the index of query q's pair, the call returns cell for cell what the bitmap call of the same mode returns
 * for that table — row ids, f32 distance bits, counts, routes — and leaves the same vss_last_exact_filtered [0..2],
 * vss_last_filter_route, vss_last_search_stats / _shape / _prescore / _prescore_descent values behind.  With lo == hi == want
 * that is also the answer of vss_search_batch_by_label.  Ranges overlap: unlike labels, the lists of one call may together
 * exceed the index's rows and take several passes (vss_last_exact_filtered [2]), as a bitmap table's do.
 * Errors: a mode other than the three (refused first, before anything is staged); no column set; lo or hi NULL with
 * n_queries > 0; those of the call of the mode.  n_queries == 0 or k == 0 returns VSS_OK.
 * The _device form takes device pointers (d_out_distances and d_out_route may be NULL), copies d_lo and d_hi back (8 bytes
 * per query) and runs on context 0.  The pipelined / multi-batch forms: vss_search_by_label_device_begin, below. */
int vss_search_batch_by_label_range(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                    const uint32_t *lo, const uint32_t *hi, int mode, uint64_t route_c, int64_t *out_rowids,
                                    float *out_distances, uint32_t *out_counts, uint8_t *out_route);
int vss_search_batch_by_label_range_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                           const uint32_t *d_lo, const uint32_t *d_hi, int mode, uint64_t route_c,
                                           int64_t *d_out_rowids, float *d_out_distances, uint32_t *d_out_counts,
                                           uint8_t *d_out_route);
/* ---- IN-list predicates on the same column (csrc/label_filter.h) ------------------------------------------------------------
 * For `items.grp IN (...)`, `items.grp = ANY(q.groups)`, `list_contains(q.groups, items.grp)` — the access-control predicate of
 * a shared store, the category list of a faceted search: the call brings `sets`, a row-major n_queries x width matrix of
 * 32-bit labels, 1 <= width <= VSS_LABEL_SET_MAX.  Query q admits a live row of id r iff 0 <= r < vss_labelled_rows(),
 * labels[r] != VSS_NO_LABEL and labels[r] == sets[q * width + j] for some j < width.
 * VSS_NO_LABEL is the padding of a shorter list: a word holding it equals nothing, and a row of the matrix that is all padding
 * is the empty predicate (count 0, ids -1, distances +inf).  Order and repeats inside a row do not change what it admits.  A
 * cell of the column holding VSS_NO_LABEL is admitted by no set: the padding does not match it.
 * The cap of 32 is a design limit, not a measurement: the test is a short loop of compares against the query's words, and beyond
 * a few dozen values a bitmap's one load per row is the cheaper test — the bitmap calls stay for that.
 * mode, route_c and out_route as for vss_search_batch_by_label.
 * Contract: with s_0 < s_1 < ... the distinct RAW rows of `sets`, ascending lexicographically as unsigned words and not
 * canonicalised (the same members in another order are another group), bitmap g = {r < labelled rows : the rule admits r for
 * s_g} and group_of[q] = the index of query q's row, the call returns cell for cell what the bitmap call of the same mode
 * returns for that table — row ids, f32 distance bits, counts, routes — and leaves the same vss_last_exact_filtered [0..2],
 * vss_last_filter_route, vss_last_search_stats / _shape / _prescore / _prescore_descent values behind.  With width 1 that is
 * also the answer of vss_search_batch_by_label, and a row of consecutive values a, a + 1, ... answers as the range does.  Sets
 * overlap: the lists of one call may together exceed the index's rows and take several passes, as a bitmap table's do.
 * Errors, in this order: a mode other than the three; width 0 or above VSS_LABEL_SET_MAX; sets NULL with n_queries > 0 (these
 * three before anything is launched or written); no column set; those of the call of the mode.  n_queries == 0 or k == 0
 * returns VSS_OK and writes nothing.
 * The _device form takes device pointers (d_out_distances and d_out_route may be NULL), copies d_sets back (4 * width bytes
 * per query) in modes exact and auto, and runs on context 0.  The pipelined / multi-batch forms: vss_search_by_label_device_begin, below. */
#define VSS_LABEL_SET_MAX 32
int vss_search_batch_by_label_set(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                  const uint32_t *sets, uint64_t width, int mode, uint64_t route_c, int64_t *out_rowids,
                                  float *out_distances, uint32_t *out_counts, uint8_t *out_route);
int vss_search_batch_by_label_set_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                         const uint32_t *d_sets, uint64_t width, int mode, uint64_t route_c,
                                         int64_t *d_out_rowids, float *d_out_distances, uint32_t *d_out_counts,
                                         uint8_t *d_out_route);
/* ---- Conjunctions of ranges over several label columns (csrc/label_filter.h) -------------------------------------------------
 * For `items.tenant = q.tenant AND items.ts >= q.since [AND items.price BETWEEN ...]`: the index keeps VSS_LABEL_COLUMNS_MAX
 * label columns, 0 .. 3.  Each is what the one column above is — one 32-bit cell per ROW ID, its own number of cells,
 * VSS_NO_LABEL where nothing was set, growth and gap fill as vss_set_labels does them — and column 0 IS that column:
 * vss_set_labels, vss_set_labels_device and vss_labelled_rows mean column 0, and the three calls above read column 0.
 * vss_set_label_column / _device write cells of one column, vss_clear_label_column frees one, vss_label_column_rows is its
 * number of cells (0 = never set, or column out of range).  A column number >= VSS_LABEL_COLUMNS_MAX is refused.  vss_clear_labels
 * and vss_load clear EVERY column; none is persisted; vss_memory_usage counts them all.  Writer lock; refused while a _begin
 * context is in flight.
 * The call: `columns` (always HOST memory) holds n_columns distinct column numbers, 1 <= n_columns <= 4, for the whole call — a
 * join's predicate has one shape for all its outer rows — and lo, hi are row-major n_queries x n_columns matrices.  Query q
 * admits a live row of id r iff for every j < n_columns, with c = columns[j]: r < vss_label_column_rows(c), cell_c[r] !=
 * VSS_NO_LABEL and lo[q, j] <= cell_c[r] <= hi[q, j], compared unsigned.  Any lo > hi makes the box empty (count 0, ids -1,
 * distances +inf); hi = 0xFFFFFFFF is "no upper bound"; `=` is lo == hi.  A column the predicate does not constrain is simply not
 * named: naming it with [0, 0xFFFFFFFF] still rejects its NULLs (VSS_NO_LABEL cells and rows beyond its cells), as SQL's
 * `x >= min` does.  mode, route_c, out_route, k and ef as for vss_search_batch_by_label_range.
 * Contract: form the n_queries x 2 n_columns matrix whose row q is (lo[q,0], hi[q,0], lo[q,1], hi[q,1], ...).  With b_0 < b_1 <
 * ... its distinct RAW rows, ascending lexicographically as unsigned words and not canonicalised (two different empty boxes are
 * two groups), bitmap g = {r : the rule admits r for b_g}, n_bits = the smallest vss_label_column_rows(c) over the named columns,
 * and group_of[q] = the index of query q's row, the call returns cell for cell what the bitmap call of the same mode returns for
 * that table — row ids, f32 distance bits, counts, routes — and leaves the same vss_last_exact_filtered [0..2],
 * vss_last_filter_route, vss_last_search_stats / _shape / _prescore / _prescore_descent values behind.  With n_columns == 1 and
 * columns = {0} that is also, counters included, the answer of vss_search_batch_by_label_range.
 * Errors, in this order, each before anything is launched or written: a mode other than the three; n_columns 0 or above 4;
 * columns NULL; a column number >= 4 or one named twice (the message names it); lo or hi NULL with n_queries > 0; a named column
 * that was never set ("no label column", with its number); those of the call of the mode.  n_queries == 0 or k == 0 returns
 * VSS_OK and writes nothing.
 * The _device form takes device pointers for everything but `columns` (d_out_distances and d_out_route may be NULL), copies d_lo
 * and d_hi back (8 * n_columns bytes per query) and runs on context 0.  The pipelined / multi-batch forms: vss_search_by_label_device_begin, below;
 * OR inside a box and more than four columns keep the bitmap calls; 64-bit columns have the box64 call below, and an IN-list
 * inside a box the set_box call below that. */
#define VSS_LABEL_COLUMNS_MAX 4
int vss_set_label_column(vss_index *index, uint32_t column, uint64_t first_rowid, const uint32_t *labels, uint64_t n);
int vss_set_label_column_device(vss_index *index, uint32_t column, uint64_t first_rowid, const uint32_t *d_labels, uint64_t n);
int vss_clear_label_column(vss_index *index, uint32_t column);
uint64_t vss_label_column_rows(const vss_index *index, uint32_t column);
int vss_search_batch_by_label_box(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                  const uint32_t *columns, uint64_t n_columns, const uint32_t *lo, const uint32_t *hi, int mode,
                                  uint64_t route_c, int64_t *out_rowids, float *out_distances, uint32_t *out_counts,
                                  uint8_t *out_route);
int vss_search_batch_by_label_box_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                         const uint32_t *columns, uint64_t n_columns, const uint32_t *d_lo, const uint32_t *d_hi,
                                         int mode, uint64_t route_c, int64_t *d_out_rowids, float *d_out_distances,
                                         uint32_t *d_out_counts, uint8_t *d_out_route);
/* ---- 64-bit label columns and boxes with 64-bit ends (csrc/label_filter.h) ------------------------------------------------------
 * For `items.tenant = q.tenant AND items.ts >= q.since` where ts is a TIMESTAMP or an id a BIGINT (INTEGRATION.md §5 has the
 * order-preserving maps to unsigned 64 bits).  Each of the VSS_LABEL_COLUMNS_MAX column slots has a WIDTH:
 * vss_label_column_width is 0 for a column without cells (or a column number out of range), 32 for one written by
 * vss_set_labels / vss_set_label_column, 64 for one written by vss_set_label_column64 / _device.  A wide column has one 64-bit
 * cell per row id, VSS_NO_LABEL64 where nothing was set; growth, gap fill and the 2^32 row-id cap are those of the narrow
 * columns, and vss_memory_usage counts 8 bytes a cell.  A column keeps its width while it has cells: a setter of the other width
 * fails with a message that names both widths (column 0 and vss_set_labels included) until vss_clear_label_column, which forgets
 * the width.  vss_clear_labels and vss_load clear wide columns like the others; none is persisted.  vss_search_batch_by_label,
 * _range, _set and _box refuse a column that is 64 bits wide ("holds 64-bit cells") and are otherwise unchanged.
 * The call: the arguments of vss_search_batch_by_label_box, but lo and hi are n_queries x n_columns matrices of uint64_t, and the
 * named columns may be of either width, mixed.  A 32-bit cell is read zero-extended, and a VSS_NO_LABEL cell reads as
 * VSS_NO_LABEL64: a 32-bit column joins a 64-bit box unchanged.  Query q admits a live row of id r iff for every j <
 * n_columns, with c = columns[j]: r < vss_label_column_rows(c), the widened cell is not VSS_NO_LABEL64, and lo[q, j] <= cell <=
 * hi[q, j], compared unsigned.  Any lo > hi empties the box; hi = 2^64 - 1 is "no upper bound" and still rejects NULLs; `=` is
 * lo == hi.  mode, route_c, out_route, k and ef as for vss_search_batch_by_label_box.
 * Contract: form the n_queries x 2 n_columns matrix of 64-bit words whose row q is (lo[q,0], hi[q,0], lo[q,1], hi[q,1], ...).
 * Its distinct RAW rows, ascending lexicographically as unsigned 64-bit words and not canonicalised, are the groups b_0 < b_1 <
 * ...; bitmap g = {r : the rule admits r for b_g}, n_bits = the smallest vss_label_column_rows(c) over the named columns, and
 * group_of[q] = the index of query q's row.  The call returns cell for cell what the bitmap call of the same mode returns for
 * that table — row ids, f32 distance bits, counts, routes — and leaves the same counters behind, as the box call does.  With
 * every named column 32 bits wide and every end below 2^32 that is also, counters included, the answer of
 * vss_search_batch_by_label_box.
 * Errors: those of the box call, in its order, except that no width is refused.  The _device form copies d_lo and d_hi back
 * (16 * n_columns bytes per query) and runs on context 0.  The pipelined / multi-batch forms: vss_search_by_label_device_begin, below; there is no
 * 64-bit equality call of its own (a box with lo == hi is the equality); the 64-bit set call is vss_search_batch_by_label_set_box
 * with n_columns == 0, below. */
#define VSS_NO_LABEL64 0xFFFFFFFFFFFFFFFFull
int vss_set_label_column64(vss_index *index, uint32_t column, uint64_t first_rowid, const uint64_t *labels, uint64_t n);
int vss_set_label_column64_device(vss_index *index, uint32_t column, uint64_t first_rowid, const uint64_t *d_labels, uint64_t n);
uint32_t vss_label_column_width(const vss_index *index, uint32_t column);
int vss_search_batch_by_label_box64(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                    const uint32_t *columns, uint64_t n_columns, const uint64_t *lo, const uint64_t *hi, int mode,
                                    uint64_t route_c, int64_t *out_rowids, float *out_distances, uint32_t *out_counts,
                                    uint8_t *out_route);
int vss_search_batch_by_label_box64_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                           const uint32_t *columns, uint64_t n_columns, const uint64_t *d_lo, const uint64_t *d_hi,
                                           int mode, uint64_t route_c, int64_t *d_out_rowids, float *d_out_distances,
                                           uint32_t *d_out_counts, uint8_t *d_out_route);
/* ---- an IN-list on one label column inside a box of ranges (csrc/label_filter.h) ------------------------------------------------
 * For `items.grp IN (the groups this user may see) AND items.ts >= q.since [AND items.price BETWEEN ...]`.  set_column is one of
 * the VSS_LABEL_COLUMNS_MAX column slots, of either width.  `sets` is a row-major n_queries x set_width matrix of uint64_t, 1 <=
 * set_width <= VSS_LABEL_SET_MAX; a shorter list is padded with VSS_NO_LABEL64.  columns[0 .. n_columns) are the RANGE columns, 0
 * <= n_columns <= 3, all distinct and none equal to set_column, of either width, mixed; lo and hi are n_queries x n_columns matrices
 * of uint64_t as in the box64 call, and with n_columns == 0 they are not read and may be NULL — that is the set call over 64-bit
 * words.  Cells are read as the box64 call reads them: a 32-bit cell zero-extended, its VSS_NO_LABEL as VSS_NO_LABEL64.
 * Query q admits a live row of id r iff r < vss_label_column_rows(c) for the set column and every named range column; the widened
 * cell of the set column is not VSS_NO_LABEL64 and equals sets[q, j] for some j < set_width; and for every range column j the
 * widened cell is not VSS_NO_LABEL64 and lo[q, j] <= cell <= hi[q, j], compared unsigned.  A padding word equals nothing: a row of
 * `sets` that is all padding is the empty predicate (count 0, ids -1), and so is any lo > hi.  Order and repeats within a row of
 * `sets` change nothing of what it admits.  A word of 2^32 or above matches no cell of a 32-bit column, and neither does
 * 0xFFFFFFFF there (the cell it would match reads as NULL).  hi == VSS_NO_LABEL64 is "no upper bound" and still rejects NULL cells.
 * A column that is not named constrains nothing.  mode, route_c, out_route, k and ef as for vss_search_batch_by_label_box64.
 * Contract: form the n_queries x (set_width + 2 n_columns) matrix of 64-bit words whose row q is (sets[q,0], ..., sets[q,w-1],
 * lo[q,0], hi[q,0], lo[q,1], hi[q,1], ...).  Its distinct RAW rows, ascending lexicographically as unsigned 64-bit words and not
 * canonicalised (the same members in another order are another group), are the groups; bitmap g = {r : the rule admits r for row
 * g}, n_bits = the smallest vss_label_column_rows(c) over the set column and the named range columns, group_of[q] = the index of
 * query q's row.  In each of the three modes the call returns cell for cell what the bitmap call of that mode returns for that
 * table — row ids, f32 distance bits, counts, routes — and leaves the same counters behind.
 * Errors, in this order: a mode other than the three; set_width 0 or above VSS_LABEL_SET_MAX; n_columns > 3; `sets` NULL with
 * n_queries > 0, or lo / hi NULL with n_queries > 0 and n_columns > 0; a bad column (set_column or a named column >=
 * VSS_LABEL_COLUMNS_MAX, a named column repeated or equal to set_column; the message names it); a column that was never set ("no
 * label column" and its number); then the errors of the mode's own call.  n_queries == 0 or k == 0 returns VSS_OK having done
 * nothing.  The _device form takes device pointers for everything but `columns` (d_out_distances and d_out_route may be NULL),
 * copies d_sets, d_lo and d_hi back (8 * (set_width + 2 n_columns) bytes per query) and runs on context 0.  The pipelined / multi-batch forms: vss_search_by_label_device_begin, below;
 * the columns are not persisted, as for its siblings.  More than one set term per
 * predicate, OR across columns and lists beyond VSS_LABEL_SET_MAX values keep the bitmap calls; a query's list is neither
 * canonicalised nor de-duplicated. */
int vss_search_batch_by_label_set_box(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                      uint32_t set_column, const uint64_t *sets, uint32_t set_width, const uint32_t *columns,
                                      uint64_t n_columns, const uint64_t *lo, const uint64_t *hi, int mode, uint64_t route_c,
                                      int64_t *out_rowids, float *out_distances, uint32_t *out_counts, uint8_t *out_route);
int vss_search_batch_by_label_set_box_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k, uint64_t ef,
                                             uint32_t set_column, const uint64_t *d_sets, uint32_t set_width, const uint32_t *columns,
                                             uint64_t n_columns, const uint64_t *d_lo, const uint64_t *d_hi, int mode,
                                             uint64_t route_c, int64_t *d_out_rowids, float *d_out_distances,
                                             uint32_t *d_out_counts, uint8_t *d_out_route);
/* Pipelined form of vss_search_batch_device: `context` (0..3) names one of the index's independent search contexts —
 * the analogue of usearch's per-thread contexts (index.hpp:2213-2240) that let several ef_search calls run
 * concurrently under the reference's shared lock (hnsw_index.cpp:388).  _begin enqueues the probe on the context's own
 * stream and returns; _end waits for it (and re-runs the rare query whose visited set overflowed).  Outputs are valid
 * after _end.  Context 0 is the one the blocking calls use. */
int vss_search_batch_device_begin(vss_index *index, int context, const float *d_queries, uint64_t n_queries, uint64_t k,
                                  uint64_t ef, int64_t *d_out_rowids, float *d_out_distances, uint32_t *d_out_counts);
/* Several probe batches answered by ONE launch of the search engine: `n_batches` (1..32; 16 until round 5) batches of `n_per_batch`
 * queries each, batch b read from d_queries[b] and answered into d_out_rowids[b] / d_out_distances[b] (entries may be
 * NULL) / d_out_counts[b]; the three tables are host arrays of device pointers, read before the call returns.  Every
 * batch gets exactly the answers vss_search_batch_device would give it.  This is what HNSW_INDEX_JOIN's Execute does
 * with the input chunks it has at hand (hnsw_optimize_join.cpp:111-168 probes them one after the other, each waiting
 * for its slowest query): the engine's walkers take queries from all of them until none is left, so the tail of one
 * batch overlaps the body of the next inside one launch.  Completed by vss_search_batch_end(context); the work
 * counters of vss_last_search_stats then cover all the batches. */
int vss_search_multi_device_begin(vss_index *index, int context, uint64_t n_batches, const float *const *d_queries,
                                  uint64_t n_per_batch, uint64_t k, uint64_t ef, int64_t *const *d_out_rowids,
                                  float *const *d_out_distances, uint32_t *const *d_out_counts);
/* Pipelined forms of vss_search_batch_filtered_device and vss_search_batch_filtered_groups_device: a pipeline thread of a
 * join with a WHERE keeps its own context, as vss_search_batch_device_begin gives an unfiltered one.  Each query gets, bit for
 * bit (row ids, f32 distance bits, count), what vss_search_batch_filtered_device returns for it alone under its own bitmap and
 * the same n_bits: tombstones excluded, rejected rows traversed, row ids >= n_bits rejected, set padding bits after n_bits
 * admit nothing, whatever follows them in memory.  Groups form: a d_group_of[q] >= n_groups is answered as the blocking
 * device form answers it — count 0, cells -1 / +inf, nothing outside the n_groups * words words read.
 * THE ONE NEW OBLIGATION: the bitmap, the table and the group numbers stay the caller's.  They must remain valid and unchanged
 * until vss_search_batch_end(context) returns — the rounds of _end that re-run a query which outgrew its scratch read them
 * again.
 * VSS_ERROR before anything is enqueued: context out of range or already in flight; a NULL query / row-id / count / bitmap
 * pointer, d_group_of NULL, n_groups == 0 or a table no size_t can hold (with n_queries and k > 0); no device memory for the
 * queries' bitmap addresses.  n_queries == 0 or k == 0: VSS_OK, nothing pending.  An empty index answers as the unfiltered
 * forms do.  A mutating call while such a probe is in flight is refused. */
int vss_search_batch_filtered_device_begin(vss_index *index, int context, const float *d_queries, uint64_t n_queries,
                                           uint64_t k, uint64_t ef, const uint64_t *d_allowed, uint64_t n_bits,
                                           int64_t *d_out_rowids, float *d_out_distances, uint32_t *d_out_counts);
int vss_search_batch_filtered_groups_device_begin(vss_index *index, int context, const float *d_queries, uint64_t n_queries,
                                                  uint64_t k, uint64_t ef, const uint64_t *d_allowed, uint64_t n_groups,
                                                  uint64_t n_bits, const uint32_t *d_group_of, int64_t *d_out_rowids,
                                                  float *d_out_distances, uint32_t *d_out_counts);
/* vss_search_multi_device_begin with predicates: every batch is one join chunk with its OWN table.  The four tables
 * d_queries / d_allowed / n_groups / d_group_of and the three output tables are host arrays of n_batches entries, read before
 * the call returns; what d_allowed[b] and d_group_of[b] point AT is device memory under the obligation above.
 *   d_allowed[b]   batch b's n_groups[b] (>= 1) bitmaps end to end, each (n_bits + 63) / 64 words; one n_bits for the launch
 *   d_group_of[b]  n_per_batch group numbers (a correlated predicate), or NULL: every query of batch b takes bitmap 0 of its
 *                  table (an uncorrelated predicate: a one-bitmap table).  Tables of different batches may be one address.
 * Every query gets what vss_search_batch_filtered_device returns for it alone under its own bitmap (the contract above); a
 * group number >= n_groups[b] gives count 0, cells -1 / +inf, and nothing outside batch b's n_groups[b] * words words is
 * read.  d_out_distances[b] may be NULL.  A launch whose batches all have d_group_of[b] == NULL and the same d_allowed[b]
 * runs as a plain one-bitmap launch.  After vss_search_batch_end, vss_last_search_stats / vss_last_search_shape / vss_timing
 * describe the launch as they do for vss_search_multi_device_begin: the counters cover all the batches.
 * VSS_ERROR before anything is enqueued, naming the batch where there is one: context out of range or already in flight;
 * n_batches outside 1..32; a NULL table array; a NULL query, row-id, count or bitmap pointer of a batch; n_groups[b] == 0; a
 * table no size_t can hold; no device memory for the queries' bitmap addresses.  n_per_batch == 0 or k == 0: VSS_OK, nothing
 * pending. */
int vss_search_multi_filtered_device_begin(vss_index *index, int context, uint64_t n_batches, const float *const *d_queries,
                                           uint64_t n_per_batch, uint64_t k, uint64_t ef, const uint64_t *const *d_allowed,
                                           const uint64_t *n_groups, uint64_t n_bits, const uint32_t *const *d_group_of,
                                           int64_t *const *d_out_rowids, float *const *d_out_distances,
                                           uint32_t *const *d_out_counts);
/* ---- Label predicates in the pipelined and multi-batch launches --------------------------------------------------------------
 * The six forms above on a caller's context (0..3), completed by vss_search_batch_end: a join's pipeline threads keep one context
 * each, several join chunks ride in one launch.  Both calls WALK THE GRAPH — mode VSS_BY_LABEL_GRAPH; there is no mode argument.
 * Modes exact and auto plan on the host (they read counts back) and stay blocking calls on context 0; label columns are still not
 * persisted.
 * vss_label_predicate names one form and carries what the form's _device call carries.  Layouts, element widths, padding words
 * (VSS_NO_LABEL / VSS_NO_LABEL64), "no upper bound" and what a query admits are exactly those of that call:
 *   VSS_LABEL_EQ       vss_search_batch_by_label_device          d_want (uint32_t)
 *   VSS_LABEL_RANGE    vss_search_batch_by_label_range_device    d_lo, d_hi (uint32_t)
 *   VSS_LABEL_SET      vss_search_batch_by_label_set_device      d_sets (uint32_t), set_width
 *   VSS_LABEL_BOX      vss_search_batch_by_label_box_device      columns, n_columns, d_lo, d_hi (uint32_t)
 *   VSS_LABEL_BOX64    vss_search_batch_by_label_box64_device    columns, n_columns, d_lo, d_hi (uint64_t)
 *   VSS_LABEL_SET_BOX  vss_search_batch_by_label_set_box_device  set_column, d_sets (uint64_t), set_width, columns, n_columns, d_lo, d_hi
 * Fields a kind does not use are ignored.  The struct and `columns` are host memory, read before the call returns; the d_ pointers
 * are device memory, read on the device only — nothing is copied back, nothing is staged, the call does not wait — and they stay
 * the caller's, valid and unchanged, until vss_search_batch_end(context) returns (its re-run rounds read the table made of them).
 * Every query gets, bit for bit (row ids, f32 distance bits, count), what the form's _device call in mode VSS_BY_LABEL_GRAPH gives
 * it, and a launch of one batch leaves the same vss_last_search_stats / _shape behind.
 * vss_search_multi_by_label_device_begin: 1..32 batches of n_per_batch queries in ONE launch, as vss_search_multi_device_begin
 * carries them; batch b brings predicates[b] with its own per-query words.  All batches of a launch share the kind, the named
 * columns in the same order (and the set column), and the set width; a launch that mixes them is refused with a message naming the
 * first batch that differs from batch 0.  d_out_distances[b] may be NULL.  The counters then cover all the batches.
 * VSS_ERROR before anything is enqueued, nothing written to the outputs: context out of range or already in flight; n_batches
 * outside 1..32; a NULL table; a kind other than the six; a mixed launch; and everything the form's blocking call refuses, in its
 * words (for the multi call with "batch b" after the entry point's name).  These checks are made whatever n_queries and k are, as
 * the blocking calls make them; with them passed, n_queries == 0 or k == 0: VSS_OK, nothing enqueued, nothing pending.  Both honour the pipelining gate below.  The writers of label columns are refused while such a probe is in
 * flight, so the columns cannot move under a launch. */
enum { VSS_LABEL_EQ = 0, VSS_LABEL_RANGE = 1, VSS_LABEL_SET = 2, VSS_LABEL_BOX = 3, VSS_LABEL_BOX64 = 4, VSS_LABEL_SET_BOX = 5 };
typedef struct vss_label_predicate {
	int kind;             /* VSS_LABEL_* */
	uint32_t set_column;  /* SET_BOX */
	uint32_t set_width;   /* SET, SET_BOX */
	uint32_t n_columns;   /* BOX, BOX64: 1..4; SET_BOX: 0..3 */
	uint32_t columns[4];  /* VSS_LABEL_COLUMNS_MAX entries, [0, n_columns) used */
	const void *d_want;   /* EQ */
	const void *d_sets;   /* SET, SET_BOX */
	const void *d_lo, *d_hi; /* RANGE, BOX, BOX64, SET_BOX */
} vss_label_predicate;
int vss_search_by_label_device_begin(vss_index *index, int context, const float *d_queries, uint64_t n_queries, uint64_t k,
                                     uint64_t ef, const vss_label_predicate *predicate, int64_t *d_out_rowids,
                                     float *d_out_distances, uint32_t *d_out_counts);
int vss_search_multi_by_label_device_begin(vss_index *index, int context, uint64_t n_batches, const float *const *d_queries,
                                           uint64_t n_per_batch, uint64_t k, uint64_t ef, const vss_label_predicate *predicates,
                                           int64_t *const *d_out_rowids, float *const *d_out_distances,
                                           uint32_t *const *d_out_counts);
int vss_search_batch_end(vss_index *index, int context);
/* Pipelining policy of the _begin calls above (default on; tuning, no reference counterpart, results never depend on it).  A launch of the search engine occupies every compute
 * unit, so a second one issued immediately would wait in its hardware queue with its clock running.  With gating on, _begin
 * returns only once the launch begun before it (on another context of this index, or by another index on the same device —
 * e.g. row-range shards sharing one GPU) has handed out its last query — the
 * moment compute units start to fall idle — or has finished; the tail of one launch still overlaps the body of the next,
 * and a launch's measured duration is execution, not queueing.  vss_set_option(index, "search.gating", 0) = issue immediately
 * (round 1's behaviour). */
/* index.ef_search(query, k, ef, thread, exact=true) — usearch search_exact_ index.hpp:4004-4019: brute force
 * over every live row.  Same output layout as vss_search_batch.  Contract, for finite inputs: the k live rows with the
 * smallest (distance, slot) pairs, in that order, distance = the engine's f32 metric (the bits vss_search_batch reports).
 * Rows are selected by MFMA ranking scores and the survivors re-scored; a query for which the engine cannot prove that this
 * selection lost no row (csrc/exact_certificate.h) is answered again by brute force in the metric itself.
 * Limits: k <= 4088; a live row whose distance is not below 3e38 (an f32 sum that overflowed: outside "finite inputs" in
 * effect) is never returned; rows wider than 10 240 dimensions cannot be answered again and fail the call (VSS_ERROR). */
int vss_search_exact_batch(vss_index *index, const float *queries, uint64_t n_queries, uint64_t k,
                           int64_t *out_rowids, float *out_distances, uint32_t *out_counts);
int vss_search_exact_batch_device(vss_index *index, const float *d_queries, uint64_t n_queries, uint64_t k,
                                  int64_t *d_out_rowids, float *d_out_distances, uint32_t *d_out_counts);
/* How many queries of the last vss_search_exact_batch* call on this index were answered again by brute force in the metric
 * because their selection by score could not be certified (diagnostics and tests; results never depend on it; 0 on data
 * whose nearest neighbours are further apart than the f32 scores' rounding error, e.g. the benchmark's). */
uint64_t vss_last_exact_fallbacks(vss_index *index);
/* Work counters of the last vss_search_batch* call, summed over its queries (usearch's
 * search_result_t::computed_distances / visited_members, index.hpp:2566-2571):
 * out[0] = computed distances, out[1] = expanded nodes, out[2] = queries, out[3] = retried queries. */
int vss_last_search_stats(vss_index *index, uint64_t *out4);
/* Shape of the search launch behind the last vss_search* call — the call's first launch; a pass that re-runs the few queries
 * which outgrew their scratch is not reported — (diagnostics and tests; no reference counterpart, results never depend on it;
 * the same context rule as vss_last_search_stats: written when the call completes):
 * out[0] = threads per workgroup, out[1] = walkers per workgroup, out[2] = workgroups, out[3] = dynamic LDS bytes per workgroup,
 * out[4] = where the candidate list lives: 0 registers, 1 LDS, 2 HBM,
 * out[5] = where the visited set lives: 0 LDS (32-bit cells), 1 LDS (compact cells), 2 HBM,
 * out[6] = 1 for the one-wave-per-query (solo) shape, out[7] = 0. */
int vss_last_search_shape(vss_index *index, uint32_t *out8);
/* Pre-scoring of the last vss_search* call (search.prescore; diagnostics and tests, results never depend on it; the same
 * context rule as vss_last_search_stats): out[0] = 1 if the call's first launch ran with the filter, out[1] = rows whose bound
 * was computed from their codes, out[2] = rows among them rejected without reading their f32 components (both summed over the
 * call's launches), out[3] = bytes of device memory the index holds for row codes (counted by vss_memory_usage). */
int vss_last_search_prescore(vss_index *index, uint64_t *out4);
/* The greedy descent's share of the above (search.prescore_descent; the same rules): out[0] = rows the descent handed to the
 * scoring waves with a finite bound (its closest distance at that hop), out[1] = rows among them that came back rejected.
 * Counted by the walkers; both are part of out[1] / out[2] of vss_last_search_prescore as well. */
int vss_last_search_prescore_descent(vss_index *index, uint64_t *out2);
/* Kernel timing measured with hipEvents on the index's stream (milliseconds): out[0] = search kernel(s) of the last
 * vss_search_batch* call, out[1] = build phase A kernels, out[2] = build phase B (link) kernels, out[3] = build host
 * wall time, out[4] = build batches, out[5] = build batches re-run with a larger visited set (cumulative since the
 * last reset). */
int vss_timing(vss_index *index, double *out6, int reset);
/* Work done by the bulk build so far (cumulative): out[0] = distances computed by the insert searches and their
 * neighbour selection (usearch add_result_t::computed_distances, index.hpp:2505-2510), out[1] = nodes expanded
 * (visited_members), out[2] = distances computed while repairing reverse links. */
int vss_build_work(vss_index *index, uint64_t *out3);
/* Per-query counters of the last host-pointer vss_search_batch call: n_queries x 2 (distances, expansions). */
int vss_last_search_query_stats(vss_index *index, uint32_t *out, uint64_t n_queries);

/* ---- maintenance ---------------------------------------------------------------------------------------- */

/* index.remove(rowid) for each id — reference HNSWIndex::Delete hnsw_index.cpp:496-512; tombstones the node
 * (key := VSS_FREE_KEY), links stay, and the slot joins the free list: later vss_stage_batch / vss_add_batch rows take
 * tombstoned slots over, in the reference's ring order, through its update() path (index_dense.hpp:1766-1793,
 * index.hpp:2801-2859) before any new slot is appended.  *out_removed = number of ids that were present.  Refused while
 * staged rows are still unlinked (the reference has no such state: every add() links immediately). */
int vss_remove_batch(vss_index *index, const int64_t *rowids, uint64_t count, uint64_t *out_removed);
/* index.compact() — reference HNSWIndex::Compact hnsw_index.cpp:481-494 -> index_dense.hpp:1479-1496 -> index_gt::compact
 * index.hpp:3405-3494.  Two effects, both computed on the device:
 *   1. the reference's reordering: every node's cluster = the node its greedy descent from the entry lands on above
 *      level 0 (search_for_one_), nodes renumbered by (level descending, cluster ascending) — ties by old slot, where the
 *      reference's std::sort is unspecified — and every neighbour slot remapped; nodes of one cluster become contiguous in
 *      HBM, so a search touches a few runs of rows instead of rows scattered over the whole table;
 *   2. the DOCUMENTED pruning (reference README.md:69 "pruning deleted items"), which usearch's compact does NOT do
 *      (DESIGN.md): tombstoned nodes are dropped, links to them removed (no new links are made; the
 *      remaining ones keep their order), the free list is emptied.
 * The entry point stays if it survives (else: the surviving node of the highest level, lowest new slot).  Answers of a
 * search are unchanged except for the order of rows at exactly equal distance.  oracle/hnsw_oracle.cpp
 * compact_reordering() / compact_dropping() are the CPU mirrors (streams compared byte for byte).
 * vss_compact_ex(reorder = 0) only prunes (survivors keep their relative order); vss_compact is vss_compact_ex(reorder = 1).
 * The surviving rows are gathered into a second vector buffer; every new array is built aside and swapped in on success,
 * so a failed call leaves the index as it was.  When the second buffer cannot be allocated the call falls back to pruning
 * with the rows moved down in place — no reordering, reported through *out_reordered (may be NULL) — and only that
 * last-resort row move cannot be undone: an error there leaves an index that must be reloaded. */
int vss_compact(vss_index *index);
int vss_compact_ex(vss_index *index, int reorder, int *out_reordered);

/* index.size() / typed size incl. tombstones / index.capacity() / index.max_level() / index.memory_usage()
 * — reference HNSWIndex::GetStats hnsw_index.cpp:292-306, GetInMemorySize.  vss_size = live rows: linked and not
 * tombstoned, plus every staged row (whether it will be appended or take over a tombstoned slot), so it does not jump at
 * vss_build_finalize; vss_nodes = slots in use, tombstones included. */
uint64_t vss_size(vss_index *index);
uint64_t vss_nodes(vss_index *index);
uint64_t vss_capacity(vss_index *index);
uint64_t vss_max_level(vss_index *index);
uint64_t vss_memory_usage(vss_index *index);
uint64_t vss_dimensions(vss_index *index);
int vss_metric(vss_index *index);
/* index.stats(level) — usearch index.hpp:3010-3027: out = {nodes, edges, max_edges, allocated_bytes}. */
int vss_level_stats(vss_index *index, uint64_t level, uint64_t *out4);
/* Progress of a running vss_build_finalize / vss_add_batch, readable from ANOTHER thread without blocking (the building
 * call holds the index meanwhile) — reference PhysicalCreateHNSWIndex::GetSinkProgress
 * hnsw_index_physical_create.cpp:312-327 (built_count against loaded_count).  *linked = rows of the current / last
 * build linked so far, *total = rows that build links. */
int vss_build_progress(vss_index *index, uint64_t *linked, uint64_t *total);

/* ---- persistence ---------------------------------------------------------------------------------------- */

/* index.save_to_stream(cb) / index.load_from_stream(cb) with the callback shape of reference
 * hnsw_index.cpp:548-551 and :234-235.  The byte stream is usearch 2.12's (index_dense.hpp:811-878), so the
 * reference's LinkedBlock writer/reader and a CPU usearch can consume it unchanged.  Callbacks return
 * non-zero on success. */
typedef int (*vss_write_cb)(void *ctx, const void *data, uint64_t size);
typedef int (*vss_read_cb)(void *ctx, void *data, uint64_t size);
uint64_t vss_serialized_length(vss_index *index);
int vss_save(vss_index *index, vss_write_cb write, void *ctx);
int vss_load(vss_index *index, vss_read_cb read, void *ctx);

/* ---- array_* scalar functions ---------------------------------------------------------------------------- */

/* array_distance / array_cosine_distance / array_negative_inner_product over `rows` FLOAT[dim] values
 * (DuckDB core functions named at reference hnsw_index.cpp:659-673).  a = rows x dim contiguous (the ARRAY child
 * vector); b = rows x dim, or ONE vector of dim floats when b_is_constant != 0.  out = rows floats.
 * Edge contract (DuckDB v1.4.3's source is not in the reference tree, so this is the engine's stated behaviour, tested in
 * tests/test_gpu_parity2.py, parity UNPINNED beyond README values):
 *   array_distance                 sqrt(sum (a-b)^2); NaN if any element is NaN; +inf if the sum overflows or an element is inf
 *   array_negative_inner_product   -(sum a*b); IEEE propagation of NaN / inf
 *   array_cosine_distance          1 - clamp(sum a*b / sqrt(sum a^2 * sum b^2), -1, 1): always within [0, 2] for finite
 *                                  non-zero inputs; NaN when either norm is zero (0/0), when an element is NaN or inf, or
 *                                  when the norm product overflows against an overflowing dot product.  (The index
 *                                  metric `cosine` special-cases zero norms as usearch does — that is a different function.) */
int vss_distance_batch(int fn, const float *a, const float *b, int b_is_constant, uint64_t rows, uint64_t dim,
                       float *out, int device);
int vss_distance_batch_device(int fn, const float *d_a, const float *d_b, int b_is_constant, uint64_t rows,
                              uint64_t dim, float *d_out, void *hip_stream);

/* ---- multi-GPU ------------------------------------------------------------------------------------------ */

/* k-way merge after the all-gather of per-shard results (row-range shards: BASELINE configs[3]; the reference has no
 * sharding, its single-index answer is dump_to's ascending (distance, key) list, hnsw_index.cpp:339, which this
 * reproduces over the union): in_* = n_shards x n_queries x k (ascending per shard, unused cells rowid -1 / +inf),
 * out_* = n_queries x k.  Device pointers, async on hip_stream. */
int vss_merge_topk_device(const float *d_in_distances, const int64_t *d_in_rowids, uint64_t n_shards,
                          uint64_t n_queries, uint64_t k, float *d_out_distances, int64_t *d_out_rowids,
                          uint32_t *d_out_counts, void *hip_stream);

/* The same merge over the PACKED exchange layout — one all-gather per launch of the search engine instead of two per
 * batch: every shard (rank) owns one block of vss_packed_block_bytes(n_queries, k) bytes holding the row ids of all the
 * launch's queries (n_queries x k int64, n_queries = batches x queries per batch, batch after batch) followed by their
 * distances (n_queries x k f32), padded to 16 bytes; `d_packed` = the n_shards blocks back to back (what
 * all_gather_into_tensor leaves), 16-byte aligned.  The engine writes a launch's answers straight into a rank's block when
 * vss_search_multi_device_begin is handed pointers into it.  Same ordering contract as above (hnsw_index.cpp:333-339). */
uint64_t vss_packed_block_bytes(uint64_t n_queries, uint64_t k);
int vss_merge_topk_packed_device(const void *d_packed, uint64_t n_shards, uint64_t n_queries, uint64_t k,
                                 float *d_out_distances, int64_t *d_out_rowids, uint32_t *d_out_counts, void *hip_stream);

/* ---- the exchange step of a sharded probe: RCCL all-gather of the packed per-shard blocks over xGMI ------------------------
 * No reference counterpart (the reference is a single-process, single-index library: SURVEY §8e); north_star's "index sharded
 * across the 8 GPUs of one node (row-range partitions, RCCL all-gather of per-shard top-k over xGMI)".  One vss_comm = one
 * rank's RCCL communicator.  RCCL is dlopen()ed on first use: libvssgpu.so has no link-time dependency on it, and a host that
 * already maps an RCCL (PyTorch) shares that copy.  Per launch of the search engine ONE collective moves every rank's block
 * (vss_packed_block_bytes(n_queries, k) bytes, filled directly by vss_search_multi_device_begin) into `gathered` (n_ranks blocks
 * back to back, rank order) on EVERY rank; vss_merge_topk_packed_device(gathered, n_ranks, ...) then merges on whichever rank
 * wants the answer.  All calls return VSS_OK / VSS_ERROR; vss_exchange_last_error() = the calling thread's last failure. */
typedef struct vss_comm vss_comm;
/* 1 if an RCCL library could be loaded (0: vss_exchange_last_error() says why; callers fall back to peer copies) */
int vss_exchange_available(void);
const char *vss_exchange_last_error(void);
/* one process per GPU (`bench.py --gpus N`, a DuckDB worker per device): rank 0 draws the 128-byte id, hands it to the others
 * out of band, and every rank calls init_rank on its own device (collective: returns when all n_ranks have called) */
int vss_exchange_unique_id(void *id128);
int vss_exchange_init_rank(vss_comm **out, int n_ranks, const void *id128, int rank, int device);
/* ONE process driving n distinct devices (host/sharded_index.hpp — the shape a DuckDB process needs): out[i] = the
 * communicator of devices[i].  Devices must be pairwise distinct (RCCL refuses two ranks on one device). */
int vss_exchange_init_all(vss_comm **out, int n, const int *devices);
/* a communicator the caller already owns (ncclComm_t, e.g. the host framework's): used, never destroyed, by this library */
int vss_exchange_adopt(vss_comm **out, void *nccl_comm, int n_ranks, int rank);
int vss_exchange_ranks(vss_comm *comm);
/* the collective: ncclAllGather(local_block -> gathered) of block_bytes bytes per rank, asynchronous on hip_stream (the
 * caller's side stream: the next launches search meanwhile).  One process holding several communicators brackets the calls
 * of one exchange with group_begin / group_end (ncclGroupStart / ncclGroupEnd). */
int vss_exchange_allgather(vss_comm *comm, const void *d_local_block, void *d_gathered, uint64_t block_bytes, void *hip_stream);
int vss_exchange_group_begin(void);
int vss_exchange_group_end(void);
int vss_exchange_destroy(vss_comm *comm);

/* Library / build identification ("gfx950", engine version). */
const char *vss_version(void);

#ifdef __cplusplus
}
#endif
#endif
