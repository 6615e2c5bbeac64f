/*
 * tgm_amd.h -- C ABI of libtgm_amd.so: the MI355X (gfx950) kernels behind the
 * drop-in hooks of tgm_amd.
 *
 * The reference (tgm-team/tgm) is pure Python/PyTorch and has no FFI of its own
 * (SURVEY.md F1), so each entry point below names the reference *Python*
 * routine it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into a contiguous buffer (the Python
 *     side passes torch.Tensor.data_ptr()); no torch types cross the boundary;
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued asynchronously, nothing here synchronises;
 *   - nothing here allocates device memory: callers pass outputs/workspaces;
 *   - return value: 0 = ok, negative = TGMX_E_* (message: tgmx_last_error()).
 *   - `status` words are device int32 bit-sets written by kernels (TGMX_ST_*),
 *     so input validation costs no host round trip; the caller reads them when
 *     it chooses to (the hooks: every call by default, or deferred).
 */
#ifndef TGM_AMD_H
#define TGM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGMX_ABI_VERSION 7

#define TGMX_OK 0
#define TGMX_E_INVALID (-1)  /* bad argument (null pointer, size, alignment) */
#define TGMX_E_LAUNCH (-2)   /* hipLaunch / runtime error                    */
#define TGMX_E_UNSUPPORTED (-3)

/* bits of a device-side status word */
#define TGMX_ST_SEED_RANGE 1 /* a hop-0 seed id outside [0, num_nodes)        */
#define TGMX_ST_SEED_TIME 2  /* a hop-0 seed time < 0                         */
#define TGMX_ST_EDGE_RANGE 4 /* an edge endpoint outside [0, num_nodes)       */
#define TGMX_ST_SCRATCH 8    /* the head of the update scratch was not zero at first use */
#define TGMX_ST_TS_BOUND 16  /* a batch timestamp outside [0, ts_bound] (tgmx_recency_step_t) */

typedef void* tgmx_stream_t;
typedef void* tgmx_event_t; /* hipEvent_t */

/* One adjacency / ring record: 16 bytes, 16-byte aligned, so one lane moves
 * one record with a single dwordx4 access. */
typedef struct tgmx_adj {
  int32_t nbr; /* neighbor node id, -1 = empty slot                          */
  int32_t eid; /* row of the resident edge_x table holding the edge features */
  int64_t ts;  /* edge timestamp                                             */
} tgmx_adj_t;

int tgmx_version(void);
/* sizeof of the argument structs as this library was compiled (a binding checks its own mirror against it):
 * 0 tgmx_adj_t, 1 tgmx_recency_step_t, 2 tgmx_tgat_layer_t, 3 tgmx_tgat_model_t, 4 tgmx_tgat_hop_t, 5 tgmx_tgat_layout_t,
 * 6 tgmx_pipeline_t, 7 tgmx_pipeline_out_t, 8 tgmx_dropout_t, 9 tgmx_tgn_memory_fwd_t, 10 tgmx_tconv_fwd_t, 11 tgmx_pipeline_post_t,
 * 12 tgmx_tgn_step_t, ..., 22 tgmx_ctan_fwd_t, 24 tgmx_gclstm_fwd_t, 26 tgmx_roland_fwd_t, 27 tgmx_decoder_fwd_t, 35 tgmx_ctan_bwd_t, 36 tgmx_graphmixer_bwd_t, 37 tgmx_dygformer_bwd_t, 38 tgmx_tpnet_bwd_t (23 and 25 are reserved and answer 0: tests/test_ctan_cpu.py and
 * tests/test_gclstm_cpu.py pin them), 28 tgmx_an_batch_t, 29 tgmx_node_analytics_t, 30 tgmx_decoder_train_t, 32 tgmx_gclstm_bwd_t (31 is
 * reserved the same way: tests/test_decoder_train_cpu.py), 39 tgmx_gcn_conv_bwd_t, 40 tgmx_tgcn_csr_fwd_t, 41 tgmx_tgcn_csr_bwd_t */
size_t tgmx_abi_sizeof(int32_t which);
const char* tgmx_last_error(void);

/* HIP timing events.  The lookup entry points accept an optional (ev_start,
 * ev_stop) pair which they record on `stream` immediately before / after their
 * kernel, so a caller can time exactly that launch on the stream it runs on
 * (bench.py's roofline leg).  tgmx_event_elapsed_ms synchronises on `stop`. */
int tgmx_event_create(tgmx_event_t* ev);
int tgmx_event_destroy(tgmx_event_t ev);
int tgmx_event_elapsed_ms(tgmx_event_t start, tgmx_event_t stop, float* ms);
int tgmx_event_synchronize(tgmx_event_t ev); /* host wait until the work recorded before `ev` is done */
/* ABI v7 -- ORDERING between two streams of one process (the loader's chain on a side stream beside the model's chain: DESIGN.md 3.3c,
 * DGDataLoader(side_stream=True)).  The reference has no counterpart: tgm/data/loader.py:158-170 runs hooks and model on one stream.
 * tgmx_event_create_sync: an event without timing (cheaper to record).  tgmx_event_record: everything enqueued on `stream` so far.
 * tgmx_stream_wait_event: work enqueued on `stream` from now on starts after the recorded work (no host wait).
 * tgmx_stream_handoff = record(ev, from) + wait(to, ev) in one call. */
int tgmx_event_create_sync(tgmx_event_t* ev);
int tgmx_event_record(tgmx_event_t ev, tgmx_stream_t stream);
int tgmx_stream_wait_event(tgmx_stream_t stream, tgmx_event_t ev);
int tgmx_stream_handoff(tgmx_stream_t from, tgmx_stream_t to, tgmx_event_t ev);

/* ------------------------------------------------------------------------
 * k-most-recent neighbor lookup over a static per-node index (CSR).
 * Replaces RecencyNeighborHook._get_recency_neighbors
 * (tgm/hooks/neighbors/recency.py:239-321) for a chronological loader whose
 * batch boundaries were known when the index was built.
 *
 *   indptr[num_nodes+1], adj[indptr[num_nodes]]: node n's entries, ordered by
 *     (batch_idx, time, role, eid); entries with eid in [ev_lo, ev_hi) are
 *     visible, of which only the last B are observable (B = max(num_nbrs)).
 *   edge_x [num_edges, D] row-major float32 (NULL iff D == 0)
 *   seeds[S] (int32; -1 = pad seed allowed iff allow_pad), qtimes[S]
 *   out_nid [S,k] int32 (pad -1), out_ts [S,k] int64 (pad 0),
 *   out_x [S,k,D] float32 (pad 0): oldest -> newest, right aligned.
 * ------------------------------------------------------------------------ */
int tgmx_recency_lookup_csr(const int64_t* indptr, const tgmx_adj_t* adj,
                            const float* edge_x, int32_t D,
                            const int32_t* seeds, const int64_t* qtimes, int64_t S,
                            int32_t k, int32_t B, int64_t ev_lo, int64_t ev_hi,
                            int32_t num_nodes, int32_t allow_pad,
                            int32_t* out_nid, int64_t* out_ts, float* out_x,
                            int32_t* status, tgmx_stream_t stream,
                            tgmx_event_t ev_start, tgmx_event_t ev_stop);

/* Uniform neighbor sampling, NeighborSamplerHook (tgm/hooks/neighbors/uniform.py:87-142) over
 * DGStorageArrayBackend.get_nbrs (tgm/core/_storage/backends/array_backend.py:108-171), against the static index built
 * with num_batches = -1.  Candidates of node n = its entries with eid < ev_hi (the hook passes the first edge whose time
 * reaches the batch's earliest timestamp: "strictly before this batch").  At most k candidates: all of them, in event
 * order, left aligned, padded with (-1, 0, 0.0) -- bit-exact with the reference.  More than k: a uniformly random
 * k-permutation without replacement (virtual Fisher-Yates), a deterministic function of (rng_seed, rng_stream, node) so
 * that every occurrence of a node in one call gets the same row, as in the reference.  The reference draws with
 * Python's Mersenne Twister (random.sample), so parity there is distributional.  k <= 64. */
int tgmx_uniform_lookup_csr(const int64_t* indptr, const tgmx_adj_t* adj, const float* edge_x, int32_t D,
                            const int32_t* seeds, int64_t S, int32_t k, int64_t ev_hi, int32_t num_nodes,
                            int32_t allow_pad, uint64_t rng_seed, uint64_t rng_stream,
                            int32_t* out_nid, int64_t* out_ts, float* out_x, int32_t* status,
                            tgmx_stream_t stream);

/* ------------------------------------------------------------------------
 * Streaming mode: per-node rings of B records, the exact state machine of the
 * reference hook (recency.py:93-102 state, :239-321 lookup, :323-399 update).
 *   ring   [num_nodes, B] records (init nbr=-1, eid=0, ts=0), write_pos[num_nodes]
 *   ring_x [num_nodes, B, D] feature row of every slot (need not be zeroed:
 *          rows of empty slots are never read)
 * ------------------------------------------------------------------------ */
int tgmx_ring_lookup(const tgmx_adj_t* ring, const int32_t* write_pos,
                     const float* ring_x, int32_t D,
                     const int32_t* seeds, const int64_t* qtimes, int64_t S,
                     int32_t k, int32_t B, int32_t num_nodes, int32_t allow_pad,
                     int32_t* out_nid, int64_t* out_ts, float* out_x,
                     int32_t* status, tgmx_stream_t stream,
                     tgmx_event_t ev_start, tgmx_event_t ev_stop);

/* Append one batch of n edges (src[i], dst[i], ts[i], edge_x[i, :]) to the rings
 * exactly as recency.py:323-399 does: stable sort of the cat[src-role, dst-role]
 * entries by key = node * (max_t + 1) + t, per-run "keep last B", scatter at
 * (write_pos + rank) % B (collisions: last wins), write_pos += kept.
 * key_wrap32 = 1 evaluates node * (max_t + 1) in int32 like the reference does
 * (recency.py:347; it wraps at dataset scale and the reference's results depend on
 * it); key_wrap32 = 0 uses int64 (the intended per-node chronological order).
 * edge_x may be NULL (rows of zeros, recency.py:325-328).  eid0 = store index of
 * the batch's first edge or -1 (recorded in the slot, informational).
 * scratch: 256-byte aligned, >= tgmx_ring_update_scratch_bytes(n, directed) bytes; its first 4096 bytes must be ZERO
 * when the buffer is first handed to the library (a self-resetting barrier of tgmx_recency_step's update workgroups
 * lives there; the library leaves it zero) -- everything behind them is plain scratch.  */
size_t tgmx_ring_update_scratch_bytes(int64_t n, int32_t directed);
int tgmx_ring_update(tgmx_adj_t* ring, int32_t* write_pos, float* ring_x, int32_t D, int32_t B,
                     int32_t num_nodes, const int32_t* src, const int32_t* dst, const int64_t* ts,
                     const float* edge_x, int64_t n, int64_t eid0, int32_t directed, int32_t key_wrap32,
                     int32_t* scratch, int32_t* status, tgmx_stream_t stream);

/* One whole hook call, RecencyNeighborHook.__call__ (recency.py:119-171), as ONE entry point: concatenate the
 * hop-0 seed groups (recency.py:173-237), run every hop's lookup (hop h+1 reads hop h's outputs in place, pads
 * included, recency.py:140-159), then append the batch to the rings (recency.py:161-163 -> :323-399).
 * Semantics are exactly tgmx_ring_lookup x n_hops followed by tgmx_ring_update (or, with indptr set,
 * tgmx_recency_lookup_csr x n_hops against the static index); the seed concatenation rides
 * on the hop-0 lookup launch (its wave of seed s reads group g's arrays and publishes seed_nid0[s] / seed_ts0[s]).
 * Scheduling (results identical): for batches of up to 4096 ring entries (2 per edge, 1 if directed) the update's
 * sort -- and up to 1024 entries also its placement decisions, which read write_pos but write only the scratch -- run
 * in extra workgroups of the hop-0 / hop-1 lookup launches; the rings themselves are written by the launch(es) that
 * follow the last lookup.  Hop 0 and hop 1 are one launch when tgmx_recency_step_plan says so (hop 1's waves re-derive
 * their seed from the unchanged rings instead of waiting for hop 0's output).
 *   timed_hop = 0 or 1 then times that one launch.
 *
 * Riders and workgroup dispatch order (what the in-kernel cross-workgroup waits rely on).  The update workgroups that ride a
 * lookup launch ("riders": one per 256-entry chunk of the batch, at most 16) meet at a barrier inside that launch: two
 * words at the head of `scratch` (arrivals, generation; self-resetting, hence "zero at first use").  A barrier between
 * workgroups of one launch is only safe if all of them are resident at the same time.  The riders are therefore the launch's
 * FIRST workgroups (blockIdx 0 .. riders - 1), and the library relies on the hardware dispatching the workgroups of a launch in
 * ascending blockIdx order: the first 16 workgroups of any launch fit the chip together (one per CU is enough), so they are
 * all dispatched before any lookup workgroup behind them can occupy a slot, whatever the grid size (tests/test_sampler_gpu.py
 * runs them in a launch 7 x larger than what the chip holds at once).  Nothing else waits across workgroups: the workgroups
 * that carry a deferred commit (tgmx_recency_step_t.defer) wait for nothing.  If the riders' barrier ever fails to complete -- a
 * scratch head that was not zero at first use, or a device that dispatched out of order -- it gives up after about a second of polling, sets
 * TGMX_ST_SCRATCH in `status` and the call's update is skipped or incomplete (the rings of that batch are then unspecified;
 * the lookups' outputs are unaffected): a reported error, never a hang (test_dirty_scratch_head_is_reported_not_hung).
 * TGMX_NO_RIDE=1 runs the same update as launches of its own (no in-kernel wait at all).
 *
 *   n_groups = 0: hop-0 seeds are already in seed_nid0 / seed_ts0 (S0 of them).
 *   n_hops   = 0: update only.          n = 0: lookups only.
 *   timed_hop >= 0: ev_start / ev_stop are recorded around that hop's lookup launch. */
#define TGMX_MAX_SEED_GROUPS 8
#define TGMX_MAX_HOPS 8
typedef struct tgmx_recency_step {
  tgmx_adj_t* ring;            /* streaming: [num_nodes, B] records.   static index: adj[M] records */
  int32_t* write_pos;          /* streaming: [num_nodes].              static index: NULL */
  float* ring_x;               /* streaming: [num_nodes, B, D].        static index: edge_x[E, D] */
  const int64_t* indptr;       /* NULL = streaming rings; else the static index (tgmx_csr_build): no update, n must be 0 */
  int64_t ev_lo, ev_hi;        /* static index: first edge visible in this epoch / first edge of this batch */
  int32_t D, B, num_nodes;
  int32_t n_groups;
  const int32_t* grp_nid[TGMX_MAX_SEED_GROUPS];
  const int64_t* grp_ts[TGMX_MAX_SEED_GROUPS];
  int64_t grp_n[TGMX_MAX_SEED_GROUPS];
  int32_t* seed_nid0;          /* [S0] hop-0 seeds (output when n_groups > 0, input otherwise) */
  int64_t* seed_ts0;           /* [S0] */
  int64_t S0;                  /* used only when n_groups == 0 */
  int32_t n_hops;
  int32_t k[TGMX_MAX_HOPS];
  int32_t* out_nid[TGMX_MAX_HOPS];  /* [S_h, k_h] */
  int64_t* out_ts[TGMX_MAX_HOPS];   /* [S_h, k_h] */
  float* out_x[TGMX_MAX_HOPS];      /* [S_h, k_h, D] */
  const int32_t* src;          /* batch edges (n = 0: no update) */
  const int32_t* dst;
  const int64_t* ts;
  const float* edge_x;         /* [n, D] or NULL */
  int64_t n, eid0;
  int32_t directed, key_wrap32;
  int32_t* scratch;            /* 256-byte aligned, >= tgmx_ring_update_scratch_bytes(n, directed) bytes */
  int32_t* status;
  int32_t timed_hop;           /* -1: none */
  tgmx_event_t ev_start, ev_stop;
  int64_t ts_bound;            /* 0 = unknown; else a promise: every timestamp of every batch satisfies 0 <= t <= ts_bound
                                  (lets the large-batch update sort only the key bits that can be set; a violation is
                                  reported as TGMX_ST_TS_BOUND and the order of that batch is unspecified) */
  /* ABI v2.  Negatives generated in place: RandomNegativeEdgeSamplerHook.__call__ (tgm/hooks/negatives/sampler.py:45-65)
   * folded into the seed fetch.  With neg_out set, seed group `neg_group` takes no id array (grp_nid[neg_group] is
   * ignored): its i-th id is the i-th draw of tgmx_random_negatives(neg_low, neg_high, ., neg_seed, neg_call) -- the
   * same counter-based generator -- its times are grp_ts[neg_group], and the hop-0 lookup also writes the group to
   * neg_out[grp_n] / neg_time_out[grp_n] (the hook's `neg` / `neg_time`).  neg_out = NULL: off (v1 behaviour). */
  int32_t neg_group, neg_low, neg_high;
  uint64_t neg_seed, neg_call;
  int32_t* neg_out;
  int64_t* neg_time_out;
  /* != 0: if the lookups of this call flag a bad hop-0 seed (TGMX_ST_SEED_RANGE / _TIME), the update of the same call leaves
   * rings and write_pos untouched -- the reference validates the seeds before it changes anything (recency.py:173-237), so a
   * caller that raises on the status word after the call (validate='sync') sees unchanged state, with ONE read-back. */
  int32_t guard_seed_errors;
  /* != 0: a promise that the batch's timestamps are non-decreasing (every batch of a chronological loader over the
   * time-sorted store): the large-batch update then takes max(ts) from the last edge instead of a reduction launch.  Checked on
   * the device: a violation is reported as TGMX_ST_TS_BOUND. */
  int32_t sorted_ts;
  /* Optional, per hop: DELTA writes of the feature rows into PERSISTENT output buffers (a loader's output pool).  A row's
   * neighbors sit at the right end of its k slots and everything left of the leftmost non-pad slot is zero, so a caller
   * that hands the same out_x[h] to consecutive calls -- unmodified in between -- and keeps out_valid[h][row] = the row's
   * SPAN (slots from its leftmost non-pad one to the end; 0 = all pads) needs writes only from slot k - max(previous span,
   * new span) on; the call updates out_valid.  Start with out_x[h] zeroed and out_valid[h] zeroed.  ~60 % of all slots
   * are pads at steady state: this halves the bytes the lookup launch writes.
   * NULL: every slot of every row is written (fresh buffers).  Ids and times are always written in full. */
  int32_t* out_valid[TGMX_MAX_HOPS];
  /* optional with out_valid: receives the span each row held BEFORE the call (the byte accounting of a timed launch needs both) */
  int32_t* out_valid_prev[TGMX_MAX_HOPS];
  /* ABI v4.  Generated negatives of a SHARD: draw i of this call is draw neg_index0 + i of the batch, so that the shares of a
   * batch drawn by different ranks are slices of the ids a single rank would draw for the whole batch (rank order concatenation
   * of the ranks' outputs then equals the single-rank tensors).  0 for an unsharded batch. */
  int64_t neg_index0;
  /* ABI v4, static index only, optional (NULL: off): int64[num_nodes], zero-initialised by the caller and owned by it.  The lookups
   * keep, per node, where its visible prefix ended the last time it was looked up, and start the next batch-boundary search there
   * (a node gains a handful of entries per batch: two probes instead of a search over its whole history).  A cache: results never
   * depend on its contents; any values are safe. */
  int64_t* csr_cursor;
  /* ABI v4, static index only.  != 0: `ring_x` holds the feature rows in ADJACENCY order -- row p belongs to adjacency record p
   * (a copy of edge_x[adj[p].eid] made once at index build) -- so a node's window of B records gathers B consecutive rows instead
   * of B rows scattered by edge id.  0: `ring_x` is edge_x[E, D], addressed by eid. */
  int32_t csr_x_by_pos;
  /* ABI v4, optional per hop: [S_h, k_h] int32, the EDGE ID behind every output slot (-1 for a pad slot; -1 everywhere for batches
   * whose edges carry no store ids, eid0 < 0).  With out_eid[h] set, out_x[h] may be NULL: the feature rows are then not copied at all
   * -- a consumer that holds the resident store (tgmx_tgat_forward: tgmx_tgat_hop_t.nbr_eid) gathers them by id where it uses them,
   * which removes the copy's writes and the consumer's re-read of them (177 of the 244 MB of a wiki-shaped batch). */
  int32_t* out_eid[TGMX_MAX_HOPS];
  /* Optional (NULL: off): DEFERRED COMMIT state of a ring (tgmx_defer_create).  With it, a call that takes the fused plan with the
   * riding placement (hops 0 + 1 as one launch, m <= 1024 entries, n_hops == 2, guard_seed_errors == 0, defer_ok != 0) does not
   * write its batch into the rings: the commit runs as extra workgroups of the NEXT such call's lookup launch, whose lookups read the
   * rings as they will be after it (an overlay: per-node headers, per-slot records, the pending batch's rows of the edge store).
   * Every other call first commits what is pending (tgmx_defer_flush).  Results are identical either way; a reader of the ring
   * state (ring, write_pos, ring_x) must flush first. */
  struct tgmx_defer* defer;
  /* != 0: this call's batch is a slice of the resident edge store -- its edge_x rows (and eid0 >= 0 ids) stay valid and unchanged
   * until the next call -- so its commit may be deferred */
  int32_t defer_ok;
} tgmx_recency_step_t;

int tgmx_recency_step(const tgmx_recency_step_t* step, tgmx_stream_t stream);
/* How tgmx_recency_step would schedule this argument block, from its sizes and pointer values alone (nothing is dereferenced, no
 * device is needed).  Informational (bench.py attributes the timed launch's bytes with bit 0; a test pins the schedule table
 * with the rest); results never depend on it.
 *   bit 0        TGMX_PLAN_FUSED01: hop 0 and hop 1 run as ONE launch (B <= 64, hop 1 not served by the narrow-row kernel;
 *                static index: wide rows only)
 *   bits 4-7     TGMX_RIDE_*: the part of the ring update that rides lookup launch 0 (hop 0, or the fused launch)
 *   bits 8-11    TGMX_RIDE_*: what rides lookup launch 1 (hop 1 when it is a launch of its own)
 *   bits 12-16   rider workgroups of launch 0        bits 17-21   rider workgroups of launch 1
 *   bits 22-23   fused launch: placement capacity of the riders' LDS (0: none, 1: 512 entries, 2: 1024 entries)
 *   bits 24-27   TGMX_AFTER_*: what follows the last lookup (a call that defers its commit, tgmx_recency_step_t.defer, leaves
 *                TGMX_AFTER_COMMIT to the next call's lookup launch; the plan does not look at `defer`)
 * The schedule, for streaming rings with n > 0, at least one hop and one seed (m = ring entries: n, or 2 n undirected; chunks =
 * ceil(m / 256); hops >= 2 carry nothing):
 *   launches         m            launch 0                   launch 1               LDS    after
 *   fused hop 0+1    <= 512       ALL x 1                    -                      512    COMMIT
 *   fused hop 0+1    513..1024    SORT_MERGE_PLACE x chunks  -                      1024   COMMIT
 *   fused hop 0+1    1025..4096   SORT_MERGE x chunks        -                      0      PRESORTED
 *   hop 0 only       <= 4096      SORT x chunks              -                      -      MERGE_PRESORTED
 *   hop 0, hop 1     <= 256       SORT_MERGE x 1             PLACE_ONLY x 1         -      COMMIT
 *   hop 0, hop 1     257..1024    SORT x chunks              MERGE_PLACE x chunks   -      COMMIT
 *   hop 0, hop 1     1025..4096   SORT x chunks              MERGE x chunks         -      PRESORTED
 * Nothing rides when there is no hop or no seed, with TGMX_NO_RIDE, or for m > 4096: TGMX_AFTER_BLOCK (m <= 4096) or
 * TGMX_AFTER_LARGE.  n = 0 and the static index: TGMX_AFTER_NONE. */
#define TGMX_PLAN_FUSED01 1
#define TGMX_RIDE_NONE 0
#define TGMX_RIDE_SORT 1             /* workgroup c sorts entries [256 c, 256 c + 256) */
#define TGMX_RIDE_MERGE 2            /* workgroup c ranks chunk c's entries among all chunks */
#define TGMX_RIDE_SORT_MERGE 3       /* both, a barrier between the riders in between */
#define TGMX_RIDE_PLACE_ONLY 4       /* one workgroup decides the placement of a merged batch */
#define TGMX_RIDE_ALL 5              /* one workgroup: chunk sorts, merge, placement decisions */
#define TGMX_RIDE_SORT_MERGE_PLACE 6 /* SORT_MERGE, then the last rider out decides the placement */
#define TGMX_RIDE_MERGE_PLACE 7      /* MERGE, then the last rider out decides the placement */
#define TGMX_AFTER_NONE 0            /* no update */
#define TGMX_AFTER_COMMIT 1          /* one launch writes what the riders decided: records, write_pos, feature rows */
#define TGMX_AFTER_PRESORTED 2       /* placement of the batch the riders sorted, then the feature rows */
#define TGMX_AFTER_MERGE_PRESORTED 3 /* the merge as a launch of its own, then TGMX_AFTER_PRESORTED */
#define TGMX_AFTER_BLOCK 4           /* the whole update of <= 4096 entries as launches of its own */
#define TGMX_AFTER_LARGE 5           /* m > 4096: the radix-sort path (its front half beside the lookups on a side stream) */
int tgmx_recency_step_plan(const tgmx_recency_step_t* step);

/* Deferred ring commit (tgmx_recency_step_t.defer): the state of one ring -- the pending batch's update arguments, the stamp
 * counter, and device buffers for both batch parities (per-node headers, per-slot records and stamps, the plan scratch: about
 * 40 bytes per ring slot, allocated on the device current at the first call that defers, freed by tgmx_defer_destroy) -- shared
 * by every argument block that carries the pointer.  TGMX_DEFER_COMMIT=0 in the environment: never defer (A/B). */
typedef struct tgmx_defer tgmx_defer_t;
tgmx_defer_t* tgmx_defer_create(int32_t num_nodes, int32_t B);
void tgmx_defer_destroy(tgmx_defer_t* d);
int tgmx_defer_pending(const tgmx_defer_t* d);
int64_t tgmx_defer_count(const tgmx_defer_t* d);       /* batches whose commit was deferred so far */         /* 1: a commit waits */
int tgmx_defer_flush(tgmx_defer_t* d, tgmx_stream_t stream); /* enqueue the pending commit (one launch) on `stream` */
/* hop-1 rows per wave of the fused hop-0 + hop-1 lookup launch from now on (0: one wave per row, the default; -1: back to
 * TGMX_FUSED_ROWS / the default); returns the previous value.  A/B and tests. */
int32_t tgmx_set_fused_rows(int32_t rows);
/* Row order of that launch's one-wave-per-row schedule from now on: 0 hop-1 rows in output order, 1 the seeds dealt round-robin
 * across equal seed groups, 2 also every seed's newest quad of rows first (-1: back to TGMX_FUSED_ORDER / the default); returns
 * the previous value.  Outputs do not depend on it.  A/B and tests. */
int32_t tgmx_set_fused_order(int32_t mode);
/* out_idx[i], i in [0, S0 * k0): the hop-1 row (s0 * k0 + j) that the i-th hop-1 wave of the launch takes under `mode`, for S0
 * hop-0 seeds in `groups` groups ending at group_end[g] (groups = 0: plain seed arrays).  Host only: the function the kernel runs. */
int32_t tgmx_fused_row_order(int64_t S0, int32_t k0, int32_t groups, const int64_t* group_end, int32_t mode, int64_t* out_idx);

/* ------------------------------------------------------------------------
 * The loader's per-batch call as ONE entry point: DGDataLoader.__call__ (tgm/data/loader.py:158-170: slice,
 * materialize) -> HookManager.execute_active_hooks (tgm/hooks/hook_manager.py:139-168) for the hook chain
 *   [EdgeShardHook (ours: a rank's contiguous share of the batch)] -> RandomNegativeEdgeSamplerHook
 *   (tgm/hooks/negatives/sampler.py:45-65) -> RecencyNeighborHook (tgm/hooks/neighbors/recency.py:119-171)
 * over the device-resident stream.  A batch is the edge range [edge_lo, edge_lo + n_edges) of the store; the seeds are
 * the roles listed in seed_role (in the order of the hook's seed_nodes_keys), every role over this rank's share
 * [n * rank / world, n * (rank + 1) / world) of the batch, all with the share's edge times as query times;
 * negatives are generated inside the seed fetch (tgmx_recency_step_t.neg_out).  Streaming mode (step.indptr == NULL,
 * update != 0) appends the WHOLE batch to the rings after the lookups (every rank replays the global batch).
 * The caller owns the outputs (a pool of preallocated buffers): nothing is allocated, nothing synchronises.
 * Results are identical to running the three hooks one by one. */
#define TGMX_SEED_SRC 0
#define TGMX_SEED_DST 1
#define TGMX_SEED_NEG 2
typedef struct tgmx_pipeline {
  const int32_t* src;          /* resident stream, time-sorted (DGData, tgm/data/dg_data.py:350-394) */
  const int32_t* dst;
  const int64_t* ts;
  const float* edge_x;         /* [num_edges, D] or NULL */
  int64_t num_edges;
  int32_t rank, world;         /* seeds come from this rank's share of every batch (world = 1: the whole batch) */
  int32_t n_roles;
  int32_t seed_role[TGMX_MAX_SEED_GROUPS]; /* TGMX_SEED_* per seed group */
  int32_t neg_low, neg_high;   /* negatives: uniform ids in [neg_low, neg_high) */
  uint64_t neg_seed;
  int32_t update;              /* streaming mode: append the batch to the rings after the lookups */
  int32_t reserved0;
  tgmx_recency_step_t step;    /* static fields filled by the caller: state pointers, D, B, num_nodes, n_hops, k[],
                                  directed, key_wrap32, scratch, status, ts_bound; static index: indptr, ev_lo
                                  (first edge visible in this epoch; ev_hi is set to edge_lo by the call) */
} tgmx_pipeline_t;

typedef struct tgmx_pipeline_out {
  int32_t* neg;                /* [share]  (NULL unless a TGMX_SEED_NEG role exists) */
  int64_t* neg_time;           /* [share] */
  int32_t* seed_nid0;          /* [n_roles * share] concatenated hop-0 seeds */
  int64_t* seed_ts0;
  int32_t* out_nid[TGMX_MAX_HOPS];
  int64_t* out_ts[TGMX_MAX_HOPS];
  float* out_x[TGMX_MAX_HOPS];
  int32_t timed_hop;           /* -1: none; else ev_start / ev_stop bracket that hop's lookup launch */
  tgmx_event_t ev_start, ev_stop;
  int32_t* out_valid[TGMX_MAX_HOPS]; /* optional: tgmx_recency_step_t.out_valid of this output set (delta feature writes) */
  int32_t* out_valid_prev[TGMX_MAX_HOPS]; /* optional: tgmx_recency_step_t.out_valid_prev */
  int32_t* out_eid[TGMX_MAX_HOPS];   /* optional: tgmx_recency_step_t.out_eid (out_x[h] may then be NULL) */
} tgmx_pipeline_out_t;

/* Optional tail of the chain, for the TGN loop: DeduplicationHook (tgm/hooks/dedup.py:35-67) over [batch src | batch dst |
 * negatives | every hop's neighbor ids] and the sampled edge list of one hop (tgmx_tgn_edge_list), enqueued behind the sampler
 * in the same call; the three sizes the host must learn (unique count, dedup status, edge count) are copied to pinned host
 * memory asynchronously and `sizes_ready` is recorded behind the copy. */
typedef struct tgmx_pipeline_post {
  int32_t dedup;               /* 1: unique ids */
  int32_t dedup_neg, dedup_nbr;/* include the negatives / the sampled neighbor ids */
  int32_t num_nodes;
  void* dedup_ws;              /* tgmx_unique_ids workspace (zero at first use) */
  int32_t* uniq_out;           /* [min(total ids, num_nodes)] */
  int32_t edge_hop;            /* -1: no edge list */
  int64_t edge_cap;            /* >= rows * k of that hop */
  int64_t* row_off;            /* [rows + 1] scratch */
  int64_t* edge_index;         /* [2, edge_cap] */
  int64_t* edge_t;             /* [edge_cap] */
  float* edge_x;               /* [edge_cap, D] */
  int64_t* dev_sizes;          /* device [3]: unique count | status (low word) | edge count; status word zero at first use */
  int64_t* host_sizes;         /* pinned host [3], device-accessible (hipHostMalloc / torch pin_memory): written by a kernel's stores */
  tgmx_event_t sizes_ready;
} tgmx_pipeline_post_t;

/* ABI v7 -- a LAUNCH WORKER: one host thread of the library that issues tgmx_pipeline_step for the caller, in submission order, on the
 * stream the caller names (the loader's side stream), bracketed by `wait_ev` (NULL or: the stream first waits for it) and `record_ev`
 * (NULL or: recorded behind the step's last launch).  The argument blocks are COPIED at submission.  tgmx_worker_wait blocks until
 * the job with that ticket has been issued (not until the device has run it) and returns ITS status (tgmx_last_error of the calling
 * thread then holds its text).  A host-side convenience with no counterpart in the reference (its loader runs in the caller's
 * thread, tgm/data/loader.py:158-170): DGDataLoader(side_stream=True) uses it so that the consumer's thread does not pay for the
 * producer's launches.  The worker issues on the device that was current when it was created. */
typedef void* tgmx_worker_t;
int tgmx_worker_create(tgmx_worker_t* w);
int tgmx_worker_destroy(tgmx_worker_t w); /* finishes the pending jobs, joins the thread */
/* Byte accounting of one lookup launch (bench / profiling), as TGMX_ACCOUNTING_PARTIALS partial triples that the caller adds
 * up whenever it likes (one launch, nothing to zero): column 0 = non-pad slots of ids[0 .. slots), column 1 = sum over rows of
 * max(span_prev, span_cur) (slots whose feature row was rewritten), column 2 = sum of span_cur.  counts: device,
 * int64[TGMX_ACCOUNTING_PARTIALS][3], overwritten.  span_* may be NULL (columns 1 and 2 are then zero). */
#define TGMX_ACCOUNTING_PARTIALS 1024
int tgmx_lookup_accounting(const int32_t* ids, int64_t slots, const int32_t* span_prev, const int32_t* span_cur, int64_t rows,
                           int64_t* counts, tgmx_stream_t stream);
int tgmx_worker_pipeline_step(tgmx_worker_t w, const tgmx_pipeline_t* pipe, int64_t edge_lo, int64_t n_edges, uint64_t neg_call,
                              const tgmx_pipeline_out_t* out, const tgmx_pipeline_post_t* post /* NULL: none */, tgmx_stream_t stream,
                              tgmx_event_t wait_ev, tgmx_event_t record_ev, uint64_t* ticket);
int tgmx_worker_wait(tgmx_worker_t w, uint64_t ticket);
int tgmx_pipeline_step(const tgmx_pipeline_t* pipe, int64_t edge_lo, int64_t n_edges, uint64_t neg_call,
                       const tgmx_pipeline_out_t* out, const tgmx_pipeline_post_t* post /* NULL: none */, tgmx_stream_t stream);

/* DGStorageArrayBackend._binary_search (tgm/core/_storage/backends/array_backend.py:301-321): event index range
 * [*lb, *ub) of the slice {start_time <= t <= end_time (inclusive; has_* = 0: unbounded), start_idx <= i < end_idx
 * (negative: unbounded)} over the time-sorted timeline.  `host_time` is a HOST array (the one exception to the
 * device-pointer convention: slicing is host arithmetic, O(log n), no device work). */
int tgmx_slice(const int64_t* host_time, int64_t n, int32_t has_start_time, int64_t start_time, int32_t has_end_time,
               int64_t end_time, int64_t start_idx, int64_t end_idx, int64_t* lb, int64_t* ub);

/* ring.fill(pad), write_pos.zero_()  (recency.py:111-117) */
int tgmx_ring_reset(tgmx_adj_t* ring, int32_t* write_pos, int32_t B, int32_t num_nodes,
                    tgmx_stream_t stream);

/* ------------------------------------------------------------------------
 * Static index build (ours: the reference has no index; SURVEY.md Appendix A.3 shows the ring state at the start of
 * a batch is a pure function of it).  Orders node n's adjacency entries by (batch_idx, time, role, eid) -- role 0 =
 * n is the source -- with one device radix sort and writes indptr[num_nodes + 1] and the 16-byte records.
 *   src/dst/ts   the time-sorted stream (the store DGData normalises, tgm/data/dg_data.py:350-394)
 *   batch_starts [num_batches] increasing first-edge indices of the loader's batches (tgm/data/loader.py:158-170);
 *                edges before batch_starts[0] form one leading batch; num_batches = -1: every edge is its own batch,
 *                i.e. plain (eid, role) order -- the candidate order of the uniform sampler (array_backend.py:127-135)
 *   directed     index source-role entries only (recency.py:332-343)
 *   workspace    >= tgmx_csr_build_workspace_bytes(num_edges, num_nodes, directed)
 *   status       TGMX_ST_EDGE_RANGE is raised for endpoints outside [0, num_nodes)
 * ------------------------------------------------------------------------ */
size_t tgmx_csr_build_workspace_bytes(int64_t num_edges, int32_t num_nodes, int32_t directed);
int tgmx_csr_build(const int32_t* src, const int32_t* dst, const int64_t* ts, int64_t num_edges, int32_t num_nodes,
                   const int64_t* batch_starts, int64_t num_batches, int32_t directed, int64_t* indptr,
                   tgmx_adj_t* adj, void* workspace, size_t workspace_bytes, int32_t* status, tgmx_stream_t stream);

/* ------------------------------------------------------------------------
 * TGAT / TemporalAttention forward (fp32, eval mode).  The attention is
 * restructured (q-length 1 => the W_KV projection folds onto the query / output
 * side, see csrc/tgat.hip); these are its building blocks, composed by
 * tgm_amd/nn/tgat.py in the order of tgm/nn/encoder/tgat.py:95-149.
 * ------------------------------------------------------------------------ */

/* nn.Dropout(p) in training mode as a counter-based mask (attention.py:119,126; PyG TransformerConv's dropout on the
 * attention weights): element i of the tensor a site covers is kept iff the 32 random bits of (seed, stream, row0 * width
 * + i) are >= floor(p * 2^32), and scaled by 1 / (1 - p).  Nothing is stored: the backward entry points regenerate the
 * mask from the same descriptor.  p = 0 (or a NULL descriptor): dropout off. */
typedef struct tgmx_dropout {
  float p;
  uint64_t seed;
  uint64_t stream; /* one value per (forward call, site) */
  int64_t row0;    /* index of the first row this call covers within the site's tensor (level-by-level calls) */
} tgmx_dropout_t;

/* out[r, c] = x[r, c] * mask(r, c) / (1 - p), c < C  (in place when out == x; forward on a tensor, backward on its gradient) */
int tgmx_dropout(const float* x, int64_t ldx, int64_t R, int32_t C, const tgmx_dropout_t* drop, float* out, int64_t ldo,
                 tgmx_stream_t stream);

/* out[n, T] = cos(fma(float(x[i]), w[t], b[t]))        Time2Vec.forward
 * (tgm/nn/modules/time_encoding.py:22-24); x is int64 (x_is_int64) or float32. */
int tgmx_time2vec(const void* x, int32_t x_is_int64, const float* w, const float* b, int32_t T,
                  int64_t n, float* out, tgmx_stream_t stream);

/* out[i, :] = table[idx[i], :], negative idx wraps (pad id -1 -> last row)
 * (tgm/nn/encoder/tgat.py:128-130 leaf features). */
int tgmx_gather_rows(const float* table, int64_t num_rows, int32_t dim, const int32_t* idx,
                     int64_t n, float* out, int64_t ldo, tgmx_stream_t stream);

/* out[R, O] = [x[:, :d] | 0 pad | time_feat]: residual / query input
 * (tgm/nn/modules/attention.py:93-95).  time_feat [R, T] may be NULL: then it is
 * Time2Vec(0) = cos(tb), what TGAT.forward passes (tgat.py:139). */
int tgmx_tgat_rres(const float* x, int64_t ldx, int32_t d, const float* tb, const float* time_feat,
                   int32_t T, int32_t O, int64_t R, float* out, int64_t ldo /* 0 = O; columns [O, ldo) zeroed */,
                   tgmx_stream_t stream);

/* (csrc/dense.hip, the dense library every model calls.)  C[b] = act(A[b] (M x K, lda) * B[b]^T (B is N x K, ldb) + bias[b]), b < batch with
 * element strides (bias: [batch, N], i.e. [N] when batch = 1); exact-fp32 MFMA.  Replaces the nn.Linear calls of
 * attention.py:96,125 and tgat.py:36-38 and the folded W_K / W_V contractions.
 * Determinism: a call is reproducible bit for bit.  The ORDER in which a row's K products are summed depends on the kernel the call
 * picks from M alone -- M <= 2048: eight contiguous K slices per output block; M >= 6144:
 * one ascending chain through 32-wide K chunks staged in LDS; otherwise four interleaved k-step sets -- so one
 * row computed in a 600-row call and in a 12 600-row call can differ in the last bits (all three are pinned against float64 in
 * tests/test_gemm_gpu.py).  Every bit-identity claim of this library (compact rows, sharded vs single-rank outputs) is between
 * calls whose M falls in the same band per GEMM; a rank whose share of a batch lands in another band is outside it --
 * TGMX_GEMM_SMALL=0 and TGMX_GEMM_LDS=0 pin the four-set kernel for every M when that matters more than the time (the 600-row
 * layer's 8 us; 15-30 % of a many-row GEMM). */
int tgmx_sgemm_nt(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                  int64_t M, int32_t N, int32_t K, const float* bias, int32_t relu, int32_t batch,
                  int64_t strideA, int64_t strideB, int64_t strideC, tgmx_stream_t stream);

/* Per-row masked softmax attention over the k sampled slots
 * (attention.py:103-122 after folding): qf [R,H,C], nbrf [R,k,d], ex [R,k,D]
 * -> zbar [R,H,C], C = d + D + T.  Neighbor time features are either computed in
 * the kernel, cos(fma(float(seed_t[r] - nbr_t[r,s]), tw, tb)) (tgat.py:143-145), or
 * read from nbr_time_feat [R,k,T] when it is non-NULL; the valid-neighbor mask is
 * nbr_id[r,s] != -1, or mask [R,k] (bytes) when it is non-NULL. */
int tgmx_tgat_attn_reduce(const float* qf, const float* nbrf, int32_t d, const float* ex, int32_t D,
                          const int64_t* seed_t, const int64_t* nbr_t, const int32_t* nbr_id,
                          const float* tw, const float* tb, const float* nbr_time_feat,
                          const uint8_t* mask, int32_t T, int32_t H, int32_t k, int64_t R,
                          float scale, int32_t head_stride /* floats between heads in qf / zbar rows, 0 = C */,
                          float* zbar, float* attn_probs /* optional [R,H,k]: softmax weights BEFORE dropout, for backward;
                                                             a row WITHOUT a valid slot stores its uniform weights negated (-1/k) */,
                          const tgmx_dropout_t* drop /* NULL = off; element (r, h, s) of [R, H, k], attention.py:119 */,
                          tgmx_stream_t stream);

/* out[R, O + d0] = [LayerNorm(y + res) * gamma + beta | z0]
 * (attention.py:127 + the concat of tgat.py:36). */
int tgmx_ln_residual_concat(const float* y, int64_t ldy, const float* res, int64_t ldr,
                            const float* gamma, const float* beta, int32_t O, float eps, const float* z0,
                            int32_t d0, int64_t R, float* out, int64_t ldo /* leading dims: 0 = dense */,
                            tgmx_stream_t stream);

/* Whole TGAT forward in one call (tgm/nn/encoder/tgat.py:95-149): enqueues the leaf gathers and,
 * per layer, the row-batched kernel sequence above.  hops[i] are the sampler's hop-i outputs
 * (rows_i = S0 * k_0 * ... * k_{i-1}); workspace from tgmx_tgat_workspace_bytes(); out [S0, emb]. */
#define TGMX_TGAT_MAX_LAYERS 4
/* Weight matrices are passed as zero-padded copies whose rows start 16-byte aligned
 * (p4(x) = x rounded up to a multiple of 4; dh = O / H; C = d + D + T): */
typedef struct tgmx_tgat_layer {
  const float* W_Q;   /* [O, p4(O)]          attn.{l}.W_Q.weight, rows padded                          */
  const float* W_K_t; /* [C, H * p4(dh)]     W_KV[:O]^T, head h's dh columns at column h * p4(dh)      */
  const float* W_V;   /* [O, p4(C)]          W_KV[O:], rows padded                                     */
  const float* W_O;   /* [O, p4(O)]                                                                    */
  const float* b_O;   /* [O]                                                                           */
  const float* ln_g;  /* [O]  layer_norm.weight                                                        */
  const float* ln_b;  /* [O]                                                                           */
  const float* fc1_w; /* [emb, p4(O + d0)]   merge_layers.{l}.fc1.weight, rows padded                  */
  const float* fc1_b; /* [emb]                                                                         */
  const float* fc2_w; /* [emb_out, p4(emb)]                                                            */
  const float* fc2_b; /* [emb_out]                                                                     */
  /* optional (inference): the query side folded onto the layer input -- qf[r, h, c] = qf_v[h*p4(C) + c] +
   * sum_j x[r, j] * qf_U[(h*p4(C) + c) * p4(d) + j], with U_h = W_K,h^T W_Q,h[:, :d] and v_h = W_K,h^T W_Q,h[:, O-T:]
   * cos(tb) (the residual's time part is Time2Vec(0), attention.py:93-95).  NULL: Q and qf are computed per call. */
  const float* qf_U;  /* [H * p4(C), p4(d)] */
  const float* qf_v;  /* [H * p4(C)]        */
  /* optional (inference): the four weights behind the attention reduce in the 16 x 16-tiled layout of tgmx_tgat_tile16()
   * (made once per parameter version).  With all four set, everything behind the attention reduce of a layer -- W_V, W_O,
   * LayerNorm(y + residual), concat, fc1 + ReLU, fc2 -- runs as ONE kernel over 16-row tiles.  NULL: the row-major copies. */
  const float* W_V_t16; /* H blocks, head h = tile16(W_KV[O + h*dh : O + (h+1)*dh], dh, C) at h * tile16_floats(dh, C) */
  const float* W_O_t16; /* tile16(W_O, O, O)                */
  const float* fc1_t16; /* tile16(fc1.weight, emb, O + d0)  */
  const float* fc2_t16; /* tile16(fc2.weight, emb_out, emb) */
  /* optional (inference, d == 1 -- a model whose nodes carry ONE feature, like the reference's example configuration): qf_U / qf_v
   * in the order the register-resident attention kernel's lanes consume them, so that the kernel evaluates qf = qf_v + x * qf_U
   * itself and the [rows, H * p4(C)] qf buffer is neither written nor read.  [H, 64, 16] floats; entry (h, lane):
   *   0..3  qf_v of the edge columns d + 4 lane + i      4..7  qf_U of the same columns
   *   8, 9  qf_v, qf_U of time column d + D + lane       10, 11  the same for time column d + D + lane + 64
   *   12, 13  qf_v, qf_U of neighbor column `lane`       14, 15  zero;   columns that do not exist: zero.       NULL: qf is a buffer. */
  const float* qf_lane;
  /* optional (inference, H == 2 and 2 * ceil(dh / 16) <= 12): both heads' W_V for the one-kernel tail's stage 1 as ONE tiled matrix --
   * tile16(S, 2 * 16 * ceil(dh / 16), C) where S stacks the heads, head h's dh rows at row h * 16 * ceil(dh / 16), zero rows between:
   * the stage then runs both heads' output blocks in one pass.  NULL: the per-head images of W_V_t16. */
  const float* W_V_t16c;
  int32_t d, D, T, O, H, emb, emb_out;
  float ln_eps;
} tgmx_tgat_layer_t;
typedef struct tgmx_tgat_model {
  const float* tw; /* [T] time_encoder.w.weight */
  const float* tb; /* [T] time_encoder.w.bias   */
  int32_t num_layers, d0;
  tgmx_tgat_layer_t layers[TGMX_TGAT_MAX_LAYERS];
  /* training (save != 0) with dropout: p and seed; `stream` = the forward call's counter -- layer j (1-based) uses
   * stream * 64 + 2 j for the attention weights and stream * 64 + 2 j + 1 for the W_O output (attention.py:119,126) */
  tgmx_dropout_t drop;
} tgmx_tgat_model_t;
typedef struct tgmx_tgat_hop {
  const int64_t* seed_t; /* [rows_i]        seed_times[i]    */
  const int32_t* nbr_id; /* [rows_i, k]     nbr_nids[i]      */
  const int64_t* nbr_t;  /* [rows_i, k]     nbr_edge_time[i] */
  const float* edge_x;   /* [rows_i, k, D]  nbr_edge_x[i]; NULL with nbr_eid set */
  int32_t k;
  /* ABI v5 (the 4 bytes of padding behind k in v4).  != 0 on hop i >= 1: a PROMISE that row r of this hop is a function of its seed
   * (hops[i-1].nbr_id[r], hops[i-1].nbr_t[r]) alone -- true when all hops come from one sampler call (hop i is seeded with hop i-1's
   * flattened outputs and no lookup of a call changes the sampler's state: tgm/hooks/neighbors/recency.py:141-143, 161-163).  Slots
   * with equal (id, time) are then the same row of every deeper level, and inference (save == 0) with every hop >= 1 so marked
   * computes each distinct row ONCE (tgmx_pair_dedup) and lets the level above read it by index -- the embeddings are the ones the
   * row-per-slot computation gives, bit for bit (a row's arithmetic does not depend on where it sits).  Pads alone -- one pair, (-1, 0)
   * -- are 35-60 % of a level at the headline shape.  0: nothing is assumed (hand-made inputs, the reference's unit tests). */
  int32_t seed_keyed;
  /* ABI v4: edge features by id.  With edge_x == NULL and nbr_eid / edge_table set, slot (r, s) reads edge_table[nbr_eid[r, s]]
   * ([E, D] rows of the resident store; -1: a pad slot, zeros) where the attention consumes it -- the sampler then never writes
   * the dense [rows, k, D] copy (tgmx_recency_step_t.out_eid) and the attention never re-reads it.  Needs the register-resident
   * attention kernel (n_heads <= 2, k <= 20, D a multiple of 4); otherwise TGMX_E_UNSUPPORTED: gather the rows first.  With save != 0
   * too (round 3, later): tgmx_tgat_backward then reads the same rows by id in its attention backward. */
  const int32_t* nbr_eid;  /* [rows_i, k] */
  const float* edge_table; /* [E, D] */
} tgmx_tgat_hop_t;
/* Where tgmx_tgat_forward keeps its intermediates (offsets in floats from the 256-byte aligned
 * workspace base; -1 = not kept).  Row strides: rres/oattn/y Op, Q H*dhp, qf/zbar H*Cp, cat Kc, h1 Ep,
 * probs H*k, out emb_out.  Level i of the hop tree occupies rows [level_off[i], level_off[i+1]). */
typedef struct tgmx_tgat_layer_layout {
  int64_t R, rres, oattn, y, Q, qf, zbar, cat, h1, probs, out;
  int32_t Op, dhp, Cp, Kc, Ep;
} tgmx_tgat_layer_layout_t;
typedef struct tgmx_tgat_layout {
  int64_t total_bytes, z0;
  int64_t level_rows[TGMX_TGAT_MAX_LAYERS + 1], level_off[TGMX_TGAT_MAX_LAYERS + 2];
  tgmx_tgat_layer_layout_t layers[TGMX_TGAT_MAX_LAYERS];
  /* ABI v5, compact rows (tgmx_tgat_hop_t.seed_keyed; -1 = level not deduplicated).  Level i's block, n = level_rows[i] int32 each:
   * [count + 15 pad | uniq n | owner n | cidx n | rep n | tgmx_pair_dedup workspace]: rep[r] = the compact row of original row r,
   * uniq[c] = the original row compact row c stands for, count = the number of compact rows (all three device-side). */
  int64_t compact[TGMX_TGAT_MAX_LAYERS + 1];
} tgmx_tgat_layout_t;
/* Weight [N, K] (row stride ldw floats) -> out[tgmx_tgat_tile16_floats(N, K)]: block (nb, kb) of 16 x 16 is 256 consecutive
 * floats, element 4 * lane + j = W[16 nb + (lane & 15)][16 kb + 4 (lane >> 4) + j], zero outside the matrix -- the order the
 * 16x16x4 fp32 MFMA's A operand is fetched in, so one wave load is 1 KB of consecutive memory. */
/* Batched 2-D repacking of small matrices -- a module's weights into the zero-padded / transposed layouts the kernels read -- as ONE
 * launch (round 3: the training step rebuilt them after every optimizer step with ~25 torch launches).  Job i writes, for r < dst_rows and
 * c < dst_cols, dst[r * dst_ld + c] = src[r * src_ld + c] (transpose == 0) or src[c * src_ld + r] (transpose != 0) where r < rows and
 * c < cols (the extent of the data in dst coordinates), 0 elsewhere.  Replaces torch.zeros + slice assignment (tgm_amd/nn/tgat.py). */
#define TGMX_PACK_MAX_JOBS 32
typedef struct tgmx_pack_job {
  const float* src;
  float* dst;
  int64_t src_ld, dst_ld;
  int32_t rows, cols, dst_rows, dst_cols;
  int32_t transpose, reserved_;
} tgmx_pack_job_t;
int tgmx_pack2d(const tgmx_pack_job_t* jobs, int32_t n_jobs, tgmx_stream_t stream);
size_t tgmx_tgat_tile16_floats(int32_t N, int32_t K);
int tgmx_tgat_tile16(const float* W, int64_t ldw, int32_t N, int32_t K, float* out, tgmx_stream_t stream);
/* ABI v5.  The distinct (id, time) pairs among n of them (one level of the hop tree; see tgmx_tgat_hop_t.seed_keyed): owner[r] = the
 * smallest index carrying r's pair, *count = number of distinct pairs, numbered densely: cidx[owner] = the pair's number (written for
 * owners only), uniq[number] = owner.  The numbering order is unspecified.  An open-addressing table in `workspace` (4-byte aligned,
 * tgmx_pair_dedup_workspace_bytes(n), contents irrelevant on entry); a memset and two launches.  n <= 2^28. */
size_t tgmx_pair_dedup_workspace_bytes(int64_t n);
int tgmx_pair_dedup(const int32_t* ids, const int64_t* times, int64_t n, int32_t* uniq, int32_t* owner, int32_t* cidx,
                    int32_t* count, void* workspace, size_t workspace_bytes, tgmx_stream_t stream);
int tgmx_tgat_layout(const tgmx_tgat_model_t* model, int64_t S0, const tgmx_tgat_hop_t* hops,
                     int32_t save, tgmx_tgat_layout_t* out);
size_t tgmx_tgat_workspace_bytes(const tgmx_tgat_model_t* model, int64_t S0, const tgmx_tgat_hop_t* hops);
/* save != 0: every layer keeps its intermediates + attention weights (training); the workspace then
 * has to be tgmx_tgat_layout(..., save=1).total_bytes large and must outlive the backward pass. */
int tgmx_tgat_forward(const tgmx_tgat_model_t* model, const float* node_x, int64_t num_nodes,
                      const int32_t* seed_ids, int64_t S0, const tgmx_tgat_hop_t* hops,
                      float* workspace, size_t workspace_bytes, int32_t save, float* out,
                      tgmx_stream_t stream);

/* ---- TGAT backward building blocks (training; composed by tgm_amd/nn/tgat.py) ---------------- */

/* C[b] (+)= A[b]^T B[b]: C[m, n] = sum_r A[r, m] * B[r, n] (weight gradients; reduction over rows),
 * exact-fp32 MFMA, deterministic two-stage reduction.  workspace: tgmx_sgemm_tn_workspace_bytes(). */
size_t tgmx_sgemm_tn_workspace_bytes(int64_t R, int32_t M, int32_t N, int32_t batch);
int tgmx_sgemm_tn(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc,
                  int64_t R, int32_t M, int32_t N, int32_t batch, int64_t strideA, int64_t strideB,
                  int64_t strideC, int32_t accumulate, float* workspace, tgmx_stream_t stream);

/* out[c] (+)= sum_r in[r * ld + c], c < C (bias / LayerNorm / Time2Vec gradients); workspace 256*C floats */
int tgmx_colsum(const float* in, int64_t ld, int64_t R, int32_t C, float* out, int32_t accumulate,
                float* workspace, tgmx_stream_t stream);

/* grad[r, c] = act[r, c] > 0 ? grad[r, c] : 0 */
int tgmx_relu_mask(float* grad, int64_t ldg, const float* act, int64_t lda, int64_t R, int32_t C,
                   tgmx_stream_t stream);

/* dst[r, c] (+)= src[r, c], c < C */
int tgmx_add_cols(float* dst, int64_t ldd, const float* src, int64_t lds, int64_t R, int32_t C,
                  int32_t accumulate, tgmx_stream_t stream);

/* LayerNorm(y + res) backward: du [R, O] (gradient of y and of res), dgx = dout * xhat (its column sum
 * is d gamma; d beta is the column sum of dout). */
int tgmx_ln_backward(const float* dout, int64_t ldd, const float* y, int64_t ldy, const float* res,
                     int64_t ldr, const float* gamma, int32_t O, float eps, int64_t R, float* du,
                     int64_t ldu, float* dgx, int64_t ldg, tgmx_stream_t stream);

/* Backward of tgmx_tgat_attn_reduce (needs the saved attention weights): given dzbar [R,H,Cs] ->
 * dqf [R,H,Cs], dnbr [R,k,d] (accumulated, may be NULL) and per-row partials dtime_rows [R, 2T] of the
 * Time2Vec weight | bias gradients (column-sum them).  k * H <= 64.
 * probs [R,H,k] as tgmx_tgat_attn_reduce saved them: weights >= 0, a masked slot exactly 0.  A row whose weights are NEGATIVE
 * (the forward writes -1/k) had no valid slot: every score was masked_fill'ed (attention.py:117), so nothing flows back through
 * the scores -- ds = 0, dqf = 0 -- and only the value path remains: dz[s] = sum_h |probs[h,s]| * mask[h,s] * dzbar[h].
 * Columns [C, head_stride) of dqf are unspecified. */
int tgmx_tgat_attn_backward(const float* qf, const float* probs, const float* dzbar, const float* nbrf,
                            int32_t d, const float* ex, int32_t D, const int64_t* seed_t,
                            const int64_t* nbr_t, const float* tw, const float* tb, int32_t T, int32_t H,
                            int32_t k, int64_t R, float scale, int32_t head_stride, float* dqf,
                            float* dnbr, float* dtime_rows, const tgmx_dropout_t* drop /* the forward's, NULL = off */,
                            tgmx_stream_t stream);

/* ---- The whole TGAT backward as ONE call (round 3) ------------------------------------------------------------------------
 * What tgm_amd/nn/_tgat_train.py composed from the building blocks above, launch by launch from Python (~100 ctypes calls and
 * ~60 torch launches per step: the training step was host-bound), driven from C++ in the same order with the same kernels -- the
 * gradients are bit-identical to the composed path (TGMX_TGAT_BWD=py keeps it for the tests), d tb to one rounding (its
 * -sin(tb) * colsum term is evaluated by our kernel instead of torch's).  `saved` is the workspace of the
 * tgmx_tgat_forward(..., save = 1) call with the same model / layout / hops; `dz` [S0, emb_out of the last layer] (row stride ldz);
 * `drop` the forward's dropout block (model->drop at that call; NULL or p = 0: off).  Every gradient has its parameter's own
 * shape, contiguous (W_KV: [2 O, C], keys then values; tw: [T]).  workspace: tgmx_tgat_backward_workspace_bytes(). */
typedef struct tgmx_tgat_layer_grads {
  float *W_Q, *W_KV, *W_O, *b_O, *ln_g, *ln_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} tgmx_tgat_layer_grads_t;
typedef struct tgmx_tgat_grads {
  float *tw, *tb;
  tgmx_tgat_layer_grads_t layers[TGMX_TGAT_MAX_LAYERS];
} tgmx_tgat_grads_t;
size_t tgmx_tgat_backward_workspace_bytes(const tgmx_tgat_model_t* model, const tgmx_tgat_layout_t* layout, const tgmx_tgat_hop_t* hops);
int tgmx_tgat_backward(const tgmx_tgat_model_t* model, const tgmx_tgat_layout_t* layout, const tgmx_tgat_hop_t* hops,
                       const float* saved, const float* dz, int64_t ldz, const tgmx_dropout_t* drop,
                       const tgmx_tgat_grads_t* grads, float* workspace, size_t workspace_bytes, tgmx_stream_t stream);

/* ------------------------------------------------------------------------
 * TGN memory module (tgm/nn/encoder/tgn.py:80-251), forward arithmetic.
 * A node's stored events ("the events of the last batch in which it appeared",
 * per role) are a window (st_lo[node], st_cnt[node]) into an append-only device log
 * {log_other int32, log_t int64, log_raw [.,D] f32}.
 * ------------------------------------------------------------------------ */

/* Replace the store of every node of a batch role (tgn.py:218-229).  Entries are given
 * in node-sorted (stable) order: perm[p] = batch entry at sorted position p, node_sorted[p]
 * its node, [left[p], right[p]) the sorted run of that node; log rows [base, base+n) are written. */
int tgmx_tgn_store(const int64_t* perm, const int32_t* node_sorted, const int64_t* left,
                   const int64_t* right, const int32_t* other, const int64_t* t, const float* raw,
                   int32_t D, int64_t n, int64_t base, int32_t* log_other, int64_t* log_t,
                   float* log_raw, int64_t* st_lo, int32_t* st_cnt, tgmx_stream_t stream);

/* aggr[r] = Last / Mean aggregation of node nodes[r]'s stored messages
 * [mem[v] | mem[other] | raw | Time2Vec(t - last_update[v])], source-role store first
 * (tgn.py:191-209, 43-74); new_lu[r] = max stored t (0 if none); aggr = 0 if none. */
int tgmx_tgn_aggregate(const int32_t* nodes, int64_t R, const float* memory,
                       const int64_t* last_update, int32_t M, int32_t num_nodes,
                       const int64_t* st_lo_s, const int32_t* st_cnt_s, const int64_t* st_lo_d,
                       const int32_t* st_cnt_d, const int32_t* log_other, const int64_t* log_t,
                       const float* log_raw, int32_t D, const float* tw, const float* tb, int32_t T,
                       int32_t mean, float* aggr, int64_t* new_lu,
                       int64_t* assoc /* optional [num_nodes]: assoc[nodes[r]] = (stamp << 32) | r, the reference's
                                         self._assoc[n_id] = arange (tgn.py:193); NULL = not recorded */,
                       int64_t stamp, tgmx_stream_t stream);

/* TGNMemory.update_state in train mode (tgn.py:165-177) when the rows of the preceding forward are at hand: the
 * reference commits _get_updated_memory(unique(src, dst)) -- for an unchanged state exactly the rows that forward produced
 * -- so the commit is memory[v] = val[row(v)], last_update[v] = lu[row(v)] with row(v) from `assoc` (stamp-checked: a
 * node that was not part of that forward sets *status to 1 and is skipped).  Duplicate nodes write identical values. */
int tgmx_tgn_commit_assoc(const int32_t* src, const int32_t* dst, int64_t n, const int64_t* assoc, int64_t stamp,
                          const float* val, const int64_t* lu, int32_t M, int32_t num_nodes, float* memory,
                          int64_t* last_update, int32_t* status, tgmx_stream_t stream);

/* TGNMemory._update_msg_store for both roles of one batch of n <= 1024 events (tgn.py:218-229, called at :173,176) in one
 * launch: log rows [base, base + n) = events grouped by src (stable), [base + n, base + 2n) grouped by dst; every node's
 * (lo, cnt) window is replaced. */
int tgmx_tgn_store_batch(const int32_t* src, const int32_t* dst, const int64_t* t, const float* raw, int32_t D, int32_t n,
                         int64_t base, int32_t* log_other, int64_t* log_t, float* log_raw, int64_t* st_lo_s,
                         int32_t* st_cnt_s, int64_t* st_lo_d, int32_t* st_cnt_d, tgmx_stream_t stream);

/* Compaction of TGNMemory's append-only message log (ours: the reference keeps a Python dict of per-node tensors, tgn.py:218-229): the live
 * windows -- (st_lo, st_cnt) per role and node -- are packed, in (role, node) order, to the front of the fresh log tensors new_*, and
 * st_lo_* are re-pointed (0 for an empty window).  The caller knows the total (the sum of the counts) and sizes new_* for it.
 * workspace >= tgmx_tgn_compact_workspace_bytes(num_nodes).  One scan + one move launch. */
size_t tgmx_tgn_compact_workspace_bytes(int32_t num_nodes);
int tgmx_tgn_compact(int64_t* st_lo_s, const int32_t* st_cnt_s, int64_t* st_lo_d, const int32_t* st_cnt_d, int32_t num_nodes,
                     const int32_t* old_other, const int64_t* old_t, const float* old_raw, int32_t D, int32_t* new_other, int64_t* new_t,
                     float* new_raw, void* workspace, size_t workspace_bytes, tgmx_stream_t stream);

/* TGNMemory._get_updated_memory (tgn.py:191-216) and GraphAttentionEmbedding.forward (tgn.py:30-40, PyG TransformerConv) as
 * ONE call each (inference / no-grad paths): the same launches, in the same order, as the building blocks above composed by
 * the host -- aggregate, gather, the two GRU GEMMs, gates; four stacked projections, edge encoding, lin_edge GEMM, segment
 * sort (or, with tgt_count / cursor / order_big, a counting grouping: histogram inside the edge encoding's launch, one scan, one placement
 * launch, segments sorted by edge id where the attention reads them -- same results), attention.  Every buffer is the caller's.  qkvs is [4, U, H*C]: query | key | value | skip; the result is its 4th
 * block (skip + attention). */
typedef struct tgmx_tgn_memory_fwd {
  const int32_t* nodes; int64_t R;
  const float* memory; const int64_t* last_update; int32_t M, num_nodes;
  const int64_t* st_lo_s; const int32_t* st_cnt_s; const int64_t* st_lo_d; const int32_t* st_cnt_d;
  const int32_t* log_other; const int64_t* log_t; const float* log_raw; int32_t D;
  const float* tw; const float* tb; int32_t T, mean;
  const float *W_ih, *b_ih, *W_hh, *b_hh;              /* GRUCell: [3M, 2M + D + T], [3M], [3M, M], [3M] */
  float *ws_aggr, *ws_h, *ws_gi, *ws_gh;               /* [R, 2M + D + T], [R, M], [R, 3M], [R, 3M] */
  float* out_mem; int64_t* out_lu;                     /* [R, M], [R] */
  int64_t* assoc; int64_t stamp;                       /* optional, as in tgmx_tgn_aggregate */
} tgmx_tgn_memory_fwd_t;
int tgmx_tgn_memory_forward(const tgmx_tgn_memory_fwd_t* args, tgmx_stream_t stream);

typedef struct tgmx_tconv_fwd {
  const float* x; int64_t U; int32_t in_ch;
  const int64_t* last_update_local;                    /* [U] */
  const int64_t* src; const int64_t* tgt; const int64_t* t; const float* msg; int64_t E; int32_t D, T;
  const float* tw; const float* tb;
  const float* W4; const float* b4; const float* W_edge; /* [4, H*C, in_ch], [4, H*C], [H*C, T + D] */
  int32_t H, C;
  float* edge_attr; float* qkvs; float* eproj;         /* [E, T + D], [4, U, H*C], [E, H*C] */
  int64_t* order; int64_t* seg_lo; int64_t* seg_hi;    /* [E], [U], [U] */
  void* sort_ws; size_t sort_ws_bytes; int32_t* status;
  /* optional (all three, or NULL: the segment-sort path): the counting grouping of the edges by target.  tgt_count [U] int32 must be
   * ZERO on entry and is left zero (the caller keeps it between calls: allocate once, zeroed); cursor [U], order_big [E] are scratch. */
  int32_t* tgt_count; int64_t* cursor; int64_t* order_big;
} tgmx_tconv_fwd_t;
int tgmx_tconv_forward(const tgmx_tconv_fwd_t* args, tgmx_stream_t stream);

/* ABI v7 -- the model side of one TGN batch as ONE call (examples/linkproppred/tgn.py:96-116 in inference order: memory(n_id) ->
 * GraphAttentionEmbedding -> memory.update_state): tgmx_tgn_memory_forward(mem), tgmx_tconv_forward(conv) with conv->x = mem->out_mem and
 * conv->last_update_local = mem->out_lu, then update_state with the rows `mem` just produced (TGNMemory.reuse_forward: tgmx_tgn_commit_assoc
 * over the batch's endpoints, mem->assoc / mem->stamp must be set) and tgmx_tgn_store_batch for the batch's n <= 1024 events.  The same
 * launches in the same order as the three module calls -- identical results -- issued back to back from C (the host side of a TGN batch
 * is ~10 us per launch when every launch is its own Python-mediated call). */
typedef struct tgmx_tgn_step {
  const tgmx_tgn_memory_fwd_t* mem;
  const tgmx_tconv_fwd_t* conv;                         /* NULL: no embedding (memory + update only) */
  const int32_t* src; const int32_t* dst; const int64_t* t; const float* raw; int32_t n;   /* the batch's events; raw [n, mem->D] */
  float* memory; int64_t* last_update; int32_t* reuse_status;                              /* written by the commit */
  int64_t log_base; int32_t* log_other; int64_t* log_t; float* log_raw;                    /* message log, rows [log_base, log_base + 2 n) */
  int64_t* st_lo_s; int32_t* st_cnt_s; int64_t* st_lo_d; int32_t* st_cnt_d;
} tgmx_tgn_step_t;
int tgmx_tgn_step(const tgmx_tgn_step_t* args, tgmx_stream_t stream);

/* The sampled edge list of one hop as the reference's TGN loop assembles it from torch ops
 * (examples/linkproppred/tgn.py:80-92): for every valid slot (nbr != -1), in slot order,
 *   edge_index[0][e] = local(seed of the row), edge_index[1][e] = local(nbr), edge_t[e] = nbr_t, edge_x[e] = nbr_x row,
 * local(v) = position of v in the sorted unique ids `uniq` (DeduplicationHook's global_to_local, tgm/hooks/dedup.py:60-66).
 * edge_index is [2, cap] (row 1 starts at cap), cap >= S * k; *count = number of edges (device); row_off: scratch [S + 1]. */
int tgmx_tgn_edge_list(const int32_t* seed, const int32_t* nbr, const int64_t* nbr_t, const float* nbr_x, int64_t S, int32_t k,
                       int32_t D, const int32_t* uniq, int64_t U, const int64_t* uniq_count /* device-side U, NULL = use U */,
                       int64_t cap, int64_t* row_off, int64_t* edge_index, int64_t* edge_t, float* edge_x, int64_t* count,
                       tgmx_stream_t stream);
/* The same with edge features BY ID (RecencyNeighborHook(edge_features='by_id'): the sampler publishes the store id of the edge behind every
 * slot, tgmx_recency_step_t.out_eid, instead of copying its feature row): edge_x[e] = edge_table[nbr_eid of the slot] -- the dense
 * [S, k, D] copies of recency.py:287-319 are never made (at the review shape: 11 MB per batch that the TGN model never reads beyond hop 0). */
int tgmx_tgn_edge_list_by_id(const int32_t* seed, const int32_t* nbr, const int64_t* nbr_t, const int32_t* nbr_eid, const float* edge_table,
                             int64_t S, int32_t k, int32_t D, const int32_t* uniq, int64_t U, const int64_t* uniq_count, int64_t cap,
                             int64_t* row_off, int64_t* edge_index, int64_t* edge_t, float* edge_x, int64_t* count, tgmx_stream_t stream);

/* torch.nn.GRUCell gates from gi = x W_ih^T + b_ih and gh = h W_hh^T + b_hh ([R, 3M], r|z|n). */
int tgmx_tgn_gru_gate(const float* gi, const float* gh, const float* h, int32_t M, int64_t R,
                      float* out, tgmx_stream_t stream);

/* memory[nodes[r]] = val[r]; last_update[nodes[r]] = lu[r] for rows with flag[r] (flag NULL: all). */
int tgmx_tgn_commit(const int32_t* nodes, const uint8_t* flag, const float* val, const int64_t* lu,
                    int32_t M, int32_t num_nodes, int64_t R, float* memory, int64_t* last_update,
                    tgmx_stream_t stream);

/* GraphAttentionEmbedding (tgn.py:14-40): edge_attr[e] = [Time2Vec(last_update_local[src[e]] - t[e]) | msg[e]] */
int tgmx_tconv_edge_attr(const int64_t* last_update_local, const int64_t* src, const int64_t* t,
                         const float* msg, const float* tw, const float* tb, int32_t T, int32_t D,
                         int64_t E, float* out, tgmx_stream_t stream);

/* Group n items by key[i] in [0, num_keys): order[] = the item ids stably sorted by key (what
 * argsort(stable=True) gives), seg_lo[k] / seg_hi[k] = the range of order[] holding key k.  Used for the incoming-edge
 * segments of TransformerConv (PyG scatter-softmax over edge_index[1]); replaces torch.sort + 2 x searchsorted.
 * Keys outside the range raise TGMX_ST_EDGE_RANGE in *status (and are clamped). */
size_t tgmx_segment_sort_workspace_bytes(int64_t n);
int tgmx_segment_sort(const int64_t* key, int64_t n, int32_t num_keys, int64_t* order, int64_t* seg_lo, int64_t* seg_hi,
                      void* workspace, size_t workspace_bytes, int32_t* status, tgmx_stream_t stream);

/* DGData.discretize's grouping, `_get_keep_indices` (tgm/data/dg_data.py:471-500), for one event group of n events:
 *   bucket[i]  = int32(floor(float64(time[i]) * factor))                                  (dg_data.py:469)
 *   key[i]     = bucket[i] * (max(id_key) + 1) + id_key[i],  id_key = id0 * (max(id0, id1) + 1) + id1 (or id0 when id1 is
 *                NULL) -- int32 arithmetic that wraps exactly like the reference's int32 tensors
 *   keep_pos   = positions of the first event of every distinct key in a STABLE sort of the keys, ascending
 *                (`reduce_op='first'`), *keep_count of them (device int64; keep_pos must hold n entries).
 * Ids must be >= 0.  workspace >= tgmx_discretize_workspace_bytes(n). */
size_t tgmx_discretize_workspace_bytes(int64_t n);
int tgmx_discretize_keep(const int64_t* time, const int32_t* id0, const int32_t* id1, int64_t n, double factor, int32_t* bucket,
                         int64_t* keep_pos, int64_t* keep_count, void* workspace, size_t workspace_bytes, tgmx_stream_t stream);

/* TransformerConv attention (third-party definition, PyG 2.6.1): for every target i,
 * out[i] += sum_j softmax_j(q_i.(k_j + e_ij)/sqrt(C)) (v_j + e_ij) per head; edges of target i are
 * order[seg_lo[i] .. seg_hi[i]) (edge ids sorted by target), src[e] = source j. */
int tgmx_tconv_attend(const float* q, const float* k, const float* v, const float* eproj,
                      const int64_t* order, const int64_t* src, const int64_t* seg_lo,
                      const int64_t* seg_hi, int64_t U, int32_t H, int32_t C, float scale, float* out,
                      const tgmx_dropout_t* drop /* training: dropout on the coefficients after the softmax, element
                                                    e * H + h (PyG TransformerConv dropout=; tgn.py:25-27 uses 0.1); NULL = off */,
                      tgmx_stream_t stream);

/* ------------------------------------------------------------------------
 * Discrete-time path (tgm/nn/encoder/tgcn.py): GCNConv normalisation + TGCN gates.
 * ------------------------------------------------------------------------ */

/* A[N, ld] (dense) = D^-1/2 (A + I) D^-1/2 with A[dst, src] = sum of the weights of edges src -> dst
 * (weight NULL = 1), self loops added where missing with weight `fill` (1, or 2 for improved=True),
 * degrees taken at the target: torch_geometric's gcn_norm (third-party to the reference).
 * workspace: 2 * N floats. */
int tgmx_gcn_norm_dense(const int64_t* src, const int64_t* dst, const float* weight, int64_t E,
                        int64_t N, float fill, int32_t add_self_loops, float* A, int64_t ld,
                        float* workspace, tgmx_stream_t stream);

/* out[N, 2C] = [a[:, :C] | b * sigmoid(gate_pre)]  (gate_pre NULL: no gating)   tgcn.py:118-149 */
int tgmx_tgcn_concat(const float* a, int64_t lda, const float* b, const float* gate_pre, int32_t C,
                     int64_t N, float* out, tgmx_stream_t stream);

/* out = sigmoid(u_pre) * H + (1 - sigmoid(u_pre)) * tanh(c_pre), n elements       tgcn.py:151-156 */
int tgmx_tgcn_output(const float* u_pre, const float* c_pre, const float* H, int64_t n, float* out,
                     tgmx_stream_t stream);

/* The whole TGCN cell forward (tgm/nn/encoder/tgcn.py:118-156, inference) as ONE call: tgmx_gcn_norm_dense, the two GEMMs of the three
 * convolutions over the shared A_hat (G = A_hat (X [W_u | W_r | W_c]^T) + [b_u | b_r | b_c]), per gate tgmx_tgcn_concat + its Linear, and
 * tgmx_tgcn_output -- the same launches in the same order as the entry points above called one by one (identical results), issued back to
 * back from C: a snapshot of a 255-node graph is 13 launches and the Python-composed sequence was host-bound at ~160 us.  Gate order
 * u, r, c everywhere.  Scratch: A [N, ldA] (ldA >= N, a multiple of 4), norm_ws [2 N], xwt [3 C, N], G [N, 3 C], cat [N, 2 C], pre [3][N, C]. */
typedef struct tgmx_tgcn_fwd {
  const float* x; int64_t N; int32_t in_ch, C;          /* node features [N, in_ch]; C = out_channels */
  const int64_t* src; const int64_t* dst; const float* edge_w; int64_t E; float fill; int32_t add_self_loops;
  const float* W3; const float* b3;                     /* stacked GCN weights [3 C, in_ch] and biases [3 C] */
  const float* lin_w[3]; const float* lin_b[3];         /* linear_{u,r,c}: [C, 2 C], [C] */
  const float* H;                                       /* [N, C] recurrent state */
  float* A; int64_t ldA; float* norm_ws; float* xwt; float* G; float* cat; float* pre[3];
  float* out;                                           /* [N, C] */
  int32_t idx32;                                        /* != 0: src / dst point at int32 ids (a DGBatch's edge_src / edge_dst as they are) */
} tgmx_tgcn_fwd_t;
int tgmx_tgcn_forward(const tgmx_tgcn_fwd_t* args, tgmx_stream_t stream);

/* Backward of the TGCN cell (tgcn.py:151-156 under loss.backward(), examples/nodeproppred/tgcn.py:92).  out = U H + (1 - U) tanh(c_pre),
 * U = sigmoid(u_pre):  du_pre = dout (H - Cc) U (1 - U), dc_pre = dout (1 - U) (1 - Cc^2), dH = dout U (n = N * C elements each). */
int tgmx_tgcn_gate_backward(const float* dout, const float* u_pre, const float* c_pre, const float* H, int64_t n, float* du_pre,
                            float* dc_pre, float* dH, tgmx_stream_t stream);
/* The gates' contributions to dH and the reset gate's pre-activation gradient.  dcat_x = dx_pre W_x are [N, 2C] (the gradient of the
 * gate's input [conv_x(X) | H] resp. [conv_c(X) | H R]); any of the three may be NULL (skipped):
 *   dcat_c: dr_pre = dcat_c[:, C:] H R (1 - R) (written when dr_pre != NULL), dH += dcat_c[:, C:] R;   dcat_u, dcat_r: dH += dcat[:, C:]. */
int tgmx_tgcn_reset_backward(const float* dcat_c, const float* dcat_u, const float* dcat_r, const float* r_pre, const float* H, int32_t C,
                             int64_t N, float* dr_pre, float* dH, tgmx_stream_t stream);

/* RandomNegativeEdgeSamplerHook (tgm/hooks/negatives/sampler.py:45-65): out_neg[i] uniform in [low, high), out_time =
 * copy of time_in (the reference: torch.randint + edge_time.clone()), one launch.  Counter-based generator keyed by
 * (seed, call, i): same distribution as the reference, a different stream than torch's. */
int tgmx_random_negatives(int32_t low, int32_t high, int64_t n, uint64_t seed, uint64_t call, int32_t* out_neg,
                          const int64_t* time_in, int64_t n_time, int64_t* out_time, tgmx_stream_t stream);
/* ABI v4: the same draws starting at index `index0` of the call's sequence (a rank's share of a sharded batch: index0 = the
 * share's offset in the batch); tgmx_random_negatives is index0 = 0. */
int tgmx_random_negatives_at(int32_t low, int32_t high, int64_t n, uint64_t seed, uint64_t call, int64_t index0, int32_t* out_neg,
                          const int64_t* time_in, int64_t n_time, int64_t* out_time, tgmx_stream_t stream);

/* DeduplicationHook (tgm/hooks/dedup.py:35-67): the sorted unique ids of up to 16 int32 id arrays (edge endpoints, extra
 * seed attributes, every hop's neighbor ids); -1 (padded slot) is skipped inside the kernel, ids outside [0, num_nodes)
 * raise TGMX_ST_SEED_RANGE.  out_ids needs room for min(total ids, num_nodes); *out_count (device) receives the number
 * written.  `parts` / `part_sizes` are HOST arrays of device pointers / lengths.  workspace: 256-byte aligned,
 * tgmx_unique_ids_workspace_bytes(num_nodes) bytes, ALL ZERO when first handed to the library (the node bitmap: every call
 * leaves it zero again, so there is no memset per call). */
size_t tgmx_unique_ids_workspace_bytes(int32_t num_nodes);
int tgmx_unique_ids(const int32_t* const* parts, const int64_t* part_sizes, int32_t num_parts, int32_t num_nodes,
                    void* workspace, int32_t* out_ids, int64_t* out_count, int32_t* status, tgmx_stream_t stream);

/* Group n <= 1024 int32 ids in one launch: stable sort by id, the permutation (sorted position -> input index), every
 * position's run [run_lo, run_hi) and a first-of-run flag; any output may be NULL.  Replaces the torch.sort +
 * searchsorted glue around the TGN message store and commit (tgm/nn/encoder/tgn.py:165-177, 218-229). */
int tgmx_group_ids(const int32_t* ids, int32_t n, int32_t* sorted, int64_t* perm, int64_t* run_lo, int64_t* run_hi,
                   uint8_t* first, tgmx_stream_t stream);
/* The same for any n (a 4096-edge batch groups 8192 endpoint ids): one stable rocPRIM radix sort (signed int32 order, like
 * torch.sort(stable=True)) + one finishing launch.  workspace: 256-byte aligned, tgmx_group_ids_workspace_bytes(n) bytes. */
size_t tgmx_group_ids_workspace_bytes(int64_t n);
int tgmx_group_ids_large(const int32_t* ids, int64_t n, int32_t* sorted, int64_t* perm, int64_t* run_lo, int64_t* run_hi,
                         uint8_t* first, void* workspace, size_t workspace_bytes, tgmx_stream_t stream);

/* ---- TGN backward building blocks (training; composed by tgm_amd/nn/_tgn_train.py).  The reference trains through
 * torch autograd (examples/linkproppred/tgn.py:97-118); memory / last_update are buffers, so the parameters reached are
 * the shared Time2Vec (tgm/nn/modules/time_encoding.py), the GRU cell and the TransformerConv projections.  The dense
 * projections differentiate through tgmx_sgemm_nt / tgmx_sgemm_tn / tgmx_colsum. ---- */

/* d(gi), d(gh) [R, 3M] of tgmx_tgn_gru_gate (torch.nn.GRUCell gate arithmetic); h is a buffer row (no dh) */
int tgmx_tgn_gru_gate_backward(const float* gi, const float* gh, const float* h, const float* dout, int32_t M, int64_t R,
                               float* dgi, float* dgh, tgmx_stream_t stream);
/* backward of tgmx_tgn_aggregate w.r.t. the Time2Vec parameters: part[r, :T] = d(tw), part[r, T:2T] = d(tb) contribution
 * of row r (same event selection as the forward; sum the rows with tgmx_colsum).  d_aggr: [R, 2M + D + T].  The row_*
 * arrays are per-row snapshots of the node's message windows and last_update taken at forward time: the reference's
 * training loop calls update_state before loss.backward() (examples/linkproppred/tgn.py:111-116). */
int tgmx_tgn_aggregate_backward(int64_t R, const int64_t* row_lo_s, const int32_t* row_cnt_s, const int64_t* row_lo_d,
                                const int32_t* row_cnt_d, const int64_t* row_last_update, const int64_t* log_t, int32_t M,
                                int32_t D, const float* tw, const float* tb, int32_t T, int32_t mean, const float* d_aggr,
                                float* part, tgmx_stream_t stream);
/* backward of tgmx_tconv_edge_attr w.r.t. the Time2Vec parameters: part [E, 2T] (d_attr: [E, T + D]) */
int tgmx_tconv_edge_attr_backward(const int64_t* last_update_local, const int64_t* src, const int64_t* t, const float* tw,
                                  const float* tb, const float* d_attr, int32_t T, int32_t D, int64_t E, float* part,
                                  tgmx_stream_t stream);
/* backward of tgmx_tconv_attend: dq written, dk / dv zero-initialised by the caller and accumulated (float atomics),
 * de [E, H*C] written for every edge.  C <= 64. */
int tgmx_tconv_attend_backward(const float* q, const float* k, const float* v, const float* eproj, const int64_t* order,
                               const int64_t* src, const int64_t* seg_lo, const int64_t* seg_hi, int64_t U, int32_t H,
                               int32_t C, float scale, const float* dout, float* dq, float* dk, float* dv, float* de,
                               const tgmx_dropout_t* drop /* the forward's, NULL = off */, tgmx_stream_t stream);

/* ---- GraphMixer (the reference's examples/linkproppred/graphmixer.py: MLPMixer link encoder + time-gap node encoder), inference ---- */

/* C = act(A B^T + bias) + res: tgmx_sgemm_nt's kernels and its M-band summation contract (one problem, no batch) with a wider epilogue:
 * act 0 = none, 1 = ReLU, 2 = exact-erf GELU (torch.nn.GELU()); res [M, N] (leading dimension ldr, may be NULL) is added after the
 * activation -- the MLPMixer's "x + FFN(x)" in the second Linear's store. */
int tgmx_sgemm_nt_ep(const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int64_t M, int32_t N, int32_t K,
                     const float* bias, int32_t act, const float* res, int64_t ldr, tgmx_stream_t stream);

/* Time-gap neighbours of a batch: the window's W edges (src / dst + e_lo, stream order) as 2 W incidences (u_j -> v_j), (v_j -> u_j),
 * stably grouped by node id: out_nbr [2 W] holds every node's neighbours in stream order (a self loop twice), and for each seed i of
 * the concatenation seeds0[:n0] | seeds1[:n1] | seeds2[:n2] its run out_nbr[out_lo[i] : out_lo[i] + out_cnt[i]].  Sizes are host
 * integers: no device -> host read.  workspace: 256-byte aligned, tgmx_time_gap_workspace_bytes(W) bytes. */
size_t tgmx_time_gap_workspace_bytes(int64_t W);
int tgmx_time_gap_group(const int32_t* src, const int32_t* dst, int64_t e_lo, int64_t W, const int32_t* seeds0, int64_t n0,
                        const int32_t* seeds1, int64_t n1, const int32_t* seeds2, int64_t n2, void* workspace, size_t workspace_bytes,
                        int32_t* out_nbr, int32_t* out_lo, int32_t* out_cnt, tgmx_stream_t stream);

/* Link-encoder prologue: out[r, :] = [edge_x[r, :D] | cos(fma(float(seed_t[r / K] - nbr_t[r]), tw, tb)) | 0 pad], r < S K, ldo >= D + T. */
int tgmx_mixer_prologue(const float* edge_x, const int64_t* seed_t, const int64_t* nbr_t, int64_t S, int32_t K, int32_t D,
                        const float* tw, const float* tb, int32_t T, float* out, int64_t ldo, tgmx_stream_t stream);

/* One MLPMixer token-mixing block on x [S, K, C] (row (s, k) at x + (s K + k) ldx): per seed and channel, LayerNorm over the K tokens
 * (tok_g / tok_b [K], biased variance), Linear K -> Ht, exact-erf GELU, Linear Ht -> K, plus the residual: z1 = x + that.  Also writes
 * y = LayerNorm over the C channels of every token of z1 (ch_g / ch_b [C]) -- the channel FFN's input.  z1 / y share the leading
 * dimension ldo.  Needs K C + (K + Ht) 128 floats of LDS per workgroup (at most 64 KiB), otherwise TGMX_E_UNSUPPORTED. */
int tgmx_mixer_token(const float* x, int64_t ldx, int64_t S, int32_t K, int32_t C, const float* tok_g, const float* tok_b,
                     const float* w1, const float* b1, int32_t Ht, const float* w2, const float* b2, const float* ch_g,
                     const float* ch_b, float eps, float* z1, float* y, int64_t ldo, tgmx_stream_t stream);

/* GraphMixer tail, one row per seed i < S (seed id: the concatenation seeds0 | seeds1 | seeds2):
 * out[i, :C] = sum_k z[i, k, :] [nbr_nids[i, k] != -1] / max(1, count), out[i, C : C + F] = mean of node_x over the seed's time-gap run
 * (0 when empty) + node_x[seed], columns [C + F, ldo) zeroed. */
int tgmx_mixer_tail(const float* z, int64_t ldz, int64_t S, int32_t K, int32_t C, const int32_t* nbr_nids, const float* node_x,
                    int64_t num_nodes, int32_t F, const int32_t* tg_nbr, const int32_t* tg_lo, const int32_t* tg_cnt,
                    const int32_t* seeds0, int64_t n0, const int32_t* seeds1, int64_t n1, const int32_t* seeds2, float* out,
                    int64_t ldo, tgmx_stream_t stream);

/* The GraphMixerEncoder inference forward as ONE call: tgmx_mixer_prologue, the projection GEMM, per layer tgmx_mixer_token and the
 * channel FFN's two GEMMs (GELU epilogue; residual epilogue), tgmx_mixer_tail and the output GEMM -- the same launches in the same order
 * as the entry points above called one by one (identical results).  Weights row-major as nn.Linear keeps them.  Scratch: x0 [S K, ldx0],
 * z / z1 / y [S K, ldz], h [S K, ldh], cat [S, ldcat]; every leading dimension a multiple of 4 (16-byte aligned GEMM operands). */
#define TGMX_MIXER_MAX_LAYERS 8
typedef struct tgmx_mixer_layer {
  const float *tok_g, *tok_b, *tok_w1, *tok_b1, *tok_w2, *tok_b2;  /* token_norm, token_feedforward.ffn.{0,3} */
  const float *ch_g, *ch_b, *ch_w1, *ch_b1, *ch_w2, *ch_b2;        /* channel_norm, channel_feedforward.ffn.{0,3} */
  int32_t tok_hidden, ch_hidden;
} tgmx_mixer_layer_t;
typedef struct tgmx_graphmixer_fwd {
  const float* nbr_edge_x; const int64_t* seed_t; const int64_t* nbr_t; const int32_t* nbr_nids;  /* hop 0: [S, K, D], [S], [S, K], [S, K] */
  const int32_t* seeds[3]; int64_t n_seeds[3];                                                     /* edge_src | edge_dst | neg */
  const int32_t* tg_nbr; const int32_t* tg_lo; const int32_t* tg_cnt;                              /* TimeGapNeighborHook */
  const float* node_x; int64_t num_nodes; int32_t F;                                               /* static node features [num_nodes, F] */
  int64_t S; int32_t K, D, T, E, num_layers; float eps;
  const float *tw, *tb, *proj_w, *proj_b, *out_w, *out_b;
  tgmx_mixer_layer_t layers[TGMX_MIXER_MAX_LAYERS];
  float *x0, *z, *z1, *y, *h, *cat; int64_t ldx0, ldz, ldh, ldcat;
  float* out;                                                                                      /* [S, E] */
} tgmx_graphmixer_fwd_t;
int tgmx_graphmixer_forward(const tgmx_graphmixer_fwd_t* args, tgmx_stream_t stream);

/* ---- GraphMixer / MLPMixer training (csrc/mixer_bwd.hip; composed by tgm_amd/nn/_graphmixer_train.py) ---- */

/* 1 when a seed's [K, C] tile with token hidden width Ht fits BOTH token kernels' LDS: the forward's 4 (K C + (K + Ht) 128) bytes and the
 * backward's 4 (4 K + 2 Ht) 33 bytes (its narrowest pass, 32 channels; it takes 128 or 64 where they fit), 64 KiB each.  The host decides the training path with this at forward time, so a forward never saves
 * for a backward that would then refuse. */
int tgmx_mixer_train_supported(int32_t K, int32_t C, int32_t Ht);

/* tgmx_mixer_token with the block's two dropout sites (training): drop_hidden after the GELU, element (s C + c) Ht + j of its stream;
 * drop_out on the block's output before the residual, element (s C + c) K + k.  NULL (or p = 0) = off; both off is tgmx_mixer_token. */
int tgmx_mixer_token_train(const float* x, int64_t ldx, int64_t S, int32_t K, int32_t C, const float* tok_g, const float* tok_b,
                           const float* w1, const float* b1, int32_t Ht, const float* w2, const float* b2, const float* ch_g,
                           const float* ch_b, float eps, float* z1, float* y, int64_t ldo, const tgmx_dropout_t* drop_hidden,
                           const tgmx_dropout_t* drop_out, tgmx_stream_t stream);

/* tgmx_graphmixer_forward in its saving form: the same launches in the same order, but layer l reads its input from save_z + l S K ldz
 * and leaves its token block's output in save_z1 + l S K ldz (args->z receives the last layer's output, args->z1 is not used; x0 and cat
 * are the caller's to keep).  drop: p, seed and the call's first stream (site s of layer l draws from stream + 4 l + s: 0 token hidden,
 * 1 token output, 2 channel hidden [S K, Hc], 3 channel output [S K, D]; row0 unused); NULL or p = 0 = off, and the results are then the
 * bits of tgmx_graphmixer_forward.  With dropout the channel sites are extra launches (tgmx_dropout in place, tgmx_add_cols). */
int tgmx_graphmixer_forward_train(const tgmx_graphmixer_fwd_t* args, float* save_z, float* save_z1, const tgmx_dropout_t* drop,
                                  tgmx_stream_t stream);

/* y[r, :] = LayerNorm over the C channels of z1[r, :] (gamma / beta [C], biased variance): what tgmx_mixer_token writes as y, recomputed
 * from the saved z1 with the same arithmetic. */
int tgmx_mixer_channel_norm(const float* z1, int64_t ldz, int64_t R, int32_t C, const float* gamma, const float* beta, float eps, float* y,
                            int64_t ldy, tgmx_stream_t stream);

/* The channel FFN's GELU backward, in place: on entry a = the pre-activations [R, C], dh = the gradient at the (dropped) hidden
 * activations; on return a = gelu(a) m, dh = dh m gelu'(a) with gelu'(a) = Phi(a) + a phi(a) (exact erf) and m the dropout scale of
 * element r C + c (drop NULL or p = 0: 1). */
int tgmx_mixer_gelu_backward(float* a, int64_t lda, float* dh, int64_t ldh, int64_t R, int32_t C, const tgmx_dropout_t* drop,
                             tgmx_stream_t stream);

/* Backward of tgmx_mixer_tail's link mean: dz[s K + k, :C] = nbr_nids[s, k] != -1 ? dcat[s, :C] / max(1, valid_s) : 0. */
int tgmx_mixer_tail_backward(const float* dcat, int64_t ldc, const int32_t* nbr_nids, int64_t S, int32_t K, int32_t C, float* dz, int64_t ldz,
                             tgmx_stream_t stream);

/* Backward of the token block z1 = x + drop_out(W2 drop_hidden(gelu(W1 LN_K(x) + b1)) + b2): one workgroup per seed, one thread per
 * channel; the column's LayerNorm, pre-activations and GELU are recomputed from x.  dx [S K, ldo] = the gradient at x (residual
 * included; must not alias dz1).  rows (may be NULL: no parameter gradient wanted) [S C, ldw], ldw >= 4 K + 2 Ht, row s C + c =
 *   [ do (K) | xn (K) | dxn (K) | dxn xhat (K) | hd (Ht) | da (Ht) | 0 ... ]
 * with do the dropped output gradient, xn the LayerNorm's output, dxn its gradient, hd the dropped hidden activations, da the gradient at
 * the pre-activations, so that
 *   d ffn.3.weight [K, Ht] = do^T hd,  d ffn.3.bias = colsum(do),  d ffn.0.weight [Ht, K] = da^T xn,  d ffn.0.bias = colsum(da),
 *   d token_norm.bias = colsum(dxn),  d token_norm.weight = colsum(dxn xhat)
 * (tgmx_sgemm_tn / tgmx_colsum over the S C rows).  Needs 4 (4 K + 2 Ht) (n + 1) bytes of LDS at n = 128, 64 or 32 channels a pass (the
 * widest that fits 64 KiB is taken), otherwise TGMX_E_UNSUPPORTED. */
int tgmx_mixer_token_backward(const float* x, int64_t ldx, const float* dz1, int64_t ldd, int64_t S, int32_t K, int32_t C, const float* tok_g,
                              const float* tok_b, const float* w1, const float* b1, int32_t Ht, const float* w2, float eps, float* dx,
                              int64_t ldo, float* rows, int64_t ldw, const tgmx_dropout_t* drop_hidden, const tgmx_dropout_t* drop_out,
                              tgmx_stream_t stream);

/* The backward of tgmx_graphmixer_forward_train as ONE call (tgmx_abi_sizeof(36)), g = dL/dout [S, E].  x0 / save_z / save_z1 / cat:
 * what that forward wrote; layers: the weights it ran with; ch_w1T [D, Hc], ch_w2T [Hc, D], out_wT [D, E] (the first D columns of out_w):
 * their transposes (one tgmx_pack2d).  Every gradient pointer may be NULL: not wanted, and the launches that feed only it are skipped;
 * gradients are written (not accumulated) in the parameters' own layouts.  No gradient reaches node_x, the edge features or the time
 * encoder.  No float atomics: two runs give the same bits.  Order:
 *   d out_w = g^T cat (tgmx_sgemm_tn), d out_b = colsum(g), dcat = g out_w[:, :D] (tgmx_sgemm_nt_ep on out_wT), tgmx_mixer_tail_backward -> gz;
 *   per layer, last first: y = tgmx_mixer_channel_norm(z1), a = y W1^T + b1 (tgmx_sgemm_nt_ep), [p > 0: gt = tgmx_dropout(gz), site 3],
 *     dh = gt W2 (tgmx_sgemm_nt_ep on ch_w2T), tgmx_mixer_gelu_backward (site 2), d ch_w2 = gt^T hd, d ch_b2 = colsum(gt), d ch_w1 = da^T y,
 *     d ch_b1 = colsum(da), dy = da W1 (tgmx_sgemm_nt_ep on ch_w1T), tgmx_ln_backward (res = a row of zeros, leading dimension 0),
 *     d ch_g = colsum(dgx), d ch_b = colsum(dy), dz1 = du + gz (tgmx_add_cols), tgmx_mixer_token_backward (sites 0, 1) -> gz and rows,
 *     the token block's six gradients from rows (two tgmx_sgemm_tn, four tgmx_colsum; Ht = 0: the two weights and ffn.0.bias are empty);
 *   d proj_w = gz^T x0 (tgmx_sgemm_tn), d proj_b = colsum(gz).
 * The chain stops at the lowest layer that still has a gradient wanted at or below it.  drop_p / drop_seed / drop_stream: the forward's. */
typedef struct tgmx_mixer_layer_grad {
  float *tok_g, *tok_b, *tok_w1, *tok_b1, *tok_w2, *tok_b2;
  float *ch_g, *ch_b, *ch_w1, *ch_b1, *ch_w2, *ch_b2;
} tgmx_mixer_layer_grad_t;
typedef struct tgmx_graphmixer_bwd {
  int64_t S; int32_t K, D, T, E, F, num_layers; float eps; float drop_p; uint64_t drop_seed, drop_stream;
  const float* g; int64_t ldg;
  const float *x0, *save_z, *save_z1, *cat; const int32_t* nbr_nids; int64_t ldx0, ldz, ldh, ldcat;
  tgmx_mixer_layer_t layers[TGMX_MIXER_MAX_LAYERS];
  const float* ch_w1T[TGMX_MIXER_MAX_LAYERS]; const float* ch_w2T[TGMX_MIXER_MAX_LAYERS]; const float* out_wT;
  float *d_proj_w, *d_proj_b, *d_out_w, *d_out_b;
  tgmx_mixer_layer_grad_t d_layers[TGMX_MIXER_MAX_LAYERS];
  void* workspace; size_t workspace_bytes;
} tgmx_graphmixer_bwd_t;
size_t tgmx_graphmixer_backward_workspace_bytes(const tgmx_graphmixer_bwd_t* args);
int tgmx_graphmixer_backward(const tgmx_graphmixer_bwd_t* args, tgmx_stream_t stream);

/* ---- DyGFormer (the reference's tgm/nn/encoder/dygformer.py), inference ---- */

/* Sequences: P (source, destination) pairs; sequence q = 2 p + side (side 0 = src[p], 1 = dst[p]) has L = k + 1 slots, slot 0 the seed
 * itself and slot j > 0 the sampler's slot j - 1 of row src_rows[p] / dst_rows[p] of the hop-0 output nbr_* [S, k(, dE)] (src_rows /
 * dst_rows NULL: rows p and P + p).  A row index outside [0, S) makes the sequence all pads.  Slot (q, j) is row q L + j of every output.
 *
 * Co-occurrence: for every slot the number of occurrences of its id in its own and in the other sequence of the pair (pads compare equal
 * in the raw count and are zeroed afterwards) -> counts [2 P L, 2] int32 (may be NULL); with feat != NULL also the encoded feature
 * feat[row, :C] = enc(own) + enc(other), enc(c) = W2 relu(w1 c + b1) + b2 read from a table over c = 0 .. L that the call fills first
 * (table: [L + 1, C] floats of scratch), columns [C, ldf) zeroed.  k < 2048.  No device -> host read. */
int tgmx_dygformer_cooccurrence(const int32_t* src, const int32_t* dst, int64_t P, const int32_t* nbr_nids, int64_t S, int32_t k,
                                const int32_t* src_rows, const int32_t* dst_rows, const float* co_w1, const float* co_b1,
                                const float* co_w2, const float* co_b2, int32_t C, float* table, int32_t* counts, float* feat,
                                int64_t ldf, tgmx_stream_t stream);

/* The node / edge / time channel inputs in one launch: node_out[row] = node_x[id] (0 for pads), edge_out[row] = nbr_x of the slot as the
 * sampler wrote it (0 in slot 0), time_out[row] = cos(fma(float(edge_time[p] - nbr_t), tw, tb)) (int64 difference, then float; slot 0:
 * 0; 0 for pads); columns past dN / dE / dT up to the leading dimensions zeroed. */
int tgmx_dygformer_prologue(const float* node_x, int64_t num_nodes, int32_t dN, const int32_t* src, const int32_t* dst,
                            const int64_t* edge_time, int64_t P, const int32_t* nbr_nids, const int64_t* nbr_t, const float* nbr_x,
                            int64_t S, int32_t k, int32_t dE, const int32_t* src_rows, const int32_t* dst_rows, const float* tw,
                            const float* tb, int32_t dT, float* node_out, int64_t ldn, float* edge_out, int64_t lde, float* time_out,
                            int64_t ldt, tgmx_stream_t stream);

/* y[r, :d] = LayerNorm(x[r, :d]) gamma + beta over the columns of each of R rows (biased variance). */
int tgmx_layernorm_rows(const float* x, int64_t ldx, int64_t R, int32_t d, const float* gamma, const float* beta, float eps, float* y,
                        int64_t ldy, tgmx_stream_t stream);

/* out[b T + i, h dh : (h + 1) dh] = softmax_j(Q_i . K_j / sqrt(dh)) V over the T rows of group b, per head h; Q / K / V are columns
 * [0, H dh), [H dh, 2 H dh), [2 H dh, 3 H dh) of qkv [B T, ldq] (nn.MultiheadAttention's in-projection output).  Exact-fp32 MFMA; scores
 * and probabilities stay in LDS / registers.  T <= 128 and dh <= 128, otherwise TGMX_E_UNSUPPORTED. */
int tgmx_mha_small(const float* qkv, int64_t ldq, int64_t B, int32_t T, int32_t H, int32_t dh, float* out, int64_t ldo,
                   tgmx_stream_t stream);

/* mean[side P + p, :D] = mean over the Np token rows (2 p + side) Np + t of x (columns [D, ldm) zeroed), then
 * out [2 P, E] = mean out_w^T + out_b: sources in rows [0, P), destinations in [P, 2 P). */
int tgmx_dygformer_tail(const float* x, int64_t ldx, int64_t P, int32_t Np, int32_t D, float* mean, int64_t ldm, const float* out_w,
                        const float* out_b, int32_t E, float* out, tgmx_stream_t stream);

/* One transformer layer on x [B T, ldx], in place: y = LN0(x); qkv = y in_w^T + in_b; att = tgmx_mha_small(qkv);
 * x1 = att out_w^T + out_b + x; y = LN1(x1); h = gelu(y w1^T + b1); x = h w2^T + b2 + x1.  Leading dimensions: multiples of 4. */
typedef struct tgmx_dygformer_layer {
  const float *ln0_g, *ln0_b, *in_w, *in_b, *out_w, *out_b;  /* norm_layers.0, multi_head_attention */
  const float *ln1_g, *ln1_b, *w1, *b1, *w2, *b2;            /* norm_layers.1, linear_layers.{0,1} */
} tgmx_dygformer_layer_t;
int tgmx_dygformer_layer(const tgmx_dygformer_layer_t* layer, int64_t B, int32_t T, int32_t H, int32_t D, float eps, float* x, float* y,
                         float* x1, float* att, int64_t ldx, float* qkv, int64_t ldq, float* h, int64_t ldh, tgmx_stream_t stream);

/* The DyGFormer inference forward as ONE call: tgmx_dygformer_cooccurrence (features), tgmx_dygformer_prologue, the four patch
 * projections (patching is a view: channel c is [2 P Np, patch ldch[c]], its GEMM writes columns [c C, (c + 1) C) of x),
 * tgmx_dygformer_layer per layer, tgmx_dygformer_tail -- the same launches in the same order as those entry points called one by one
 * (identical results).  proj_w[c]: [C, patch ldch[c]] (each slot's columns zero-padded to ldch[c]).  Scratch: table [(k + 2) C],
 * ch[c] [2 P L, ldch[c]], x / y / x1 / att [2 P Np, ldx], mean [2 P, ldx], qkv [2 P Np, ldq], h [2 P Np, ldh]. */
#define TGMX_DYGFORMER_MAX_LAYERS 8
typedef struct tgmx_dygformer_fwd {
  const float* node_x; int64_t num_nodes;
  const int32_t *src, *dst; const int64_t* edge_time; int64_t P;
  const int32_t* nbr_nids; const int64_t* nbr_t; const float* nbr_x; int64_t S;  /* hop 0: [S, k], [S, k], [S, k, dE] */
  const int32_t *src_rows, *dst_rows;                                            /* [P] rows of hop 0, or NULL */
  int32_t k, dN, dE, dT, C, patch, heads, E, num_layers; float eps;
  const float *tw, *tb, *co_w1, *co_b1, *co_w2, *co_b2;
  const float* proj_w[4]; const float* proj_b[4];                                /* node, edge, time, co-occurrence */
  const float *out_w, *out_b;
  tgmx_dygformer_layer_t layers[TGMX_DYGFORMER_MAX_LAYERS];
  float* table; float* ch[4]; int64_t ldch[4];
  float *x, *y, *x1, *att, *qkv, *h, *mean; int64_t ldx, ldq, ldh;
  float* out;                                                                    /* [2 P, E] */
} tgmx_dygformer_fwd_t;
int tgmx_dygformer_forward(const tgmx_dygformer_fwd_t* args, tgmx_stream_t stream);

/* ---- DyGFormer / TransformerEncoder training (csrc/dygformer_bwd.hip; composed by tgm_amd/nn/_dygformer_train.py) ---- */

/* 1 when T tokens at head dimension dh fit the attention BACKWARD's LDS plan: Q, K, V, dO [Tp, ldk] and two T x T tiles (the dropped
 * probabilities and dS) all resident, Tp = T rounded up to 16, ldk as the forward's, the tiles' pitches 16 and 18 (mod 32) floats, 160 KiB
 * at most; T <= 128, dh <= 128.  (64, 100) takes 140.5 KiB -- one workgroup per CU.  (64, 128) and (128, 32) are outside: the training
 * envelope is narrower than inference's.  The host decides the training path with this at forward time, so a forward never saves for a
 * backward that would then refuse. */
int tgmx_mha_small_train_supported(int32_t T, int32_t dh);

/* tgmx_mha_small with dropout on the normalised probabilities before the P V product (nn.MultiheadAttention's): element
 * ((b H + h) T + i) T + j of drop's stream.  NULL or p = 0: tgmx_mha_small, bit for bit. */
int tgmx_mha_small_train(const float* qkv, int64_t ldq, int64_t B, int32_t T, int32_t H, int32_t dh, float* out, int64_t ldo,
                         const tgmx_dropout_t* drop, tgmx_stream_t stream);

/* Backward of tgmx_mha_small_train: qkv as the forward read it, datt [B T, ldo] the gradient at its output, drop the forward's descriptor
 * -> dqkv [B T, ldq], columns dQ | dK | dV laid out as qkv's (columns [3 H dh, ldq) untouched).  One workgroup per (group, head); the
 * probabilities are recomputed in LDS with the forward's arithmetic, nothing T x T reaches memory:
 *   dV = (P o m)^T dO,  dP = (dO V^T) o m,  dS = P o (dP - rowsum(dP o P)),  dQ = scale dS K,  dK = scale dS^T Q
 * on the exact-fp32 MFMA.  No atomics; every element written once; two runs give the same bits.  Outside
 * tgmx_mha_small_train_supported: TGMX_E_UNSUPPORTED. */
int tgmx_mha_small_backward(const float* qkv, int64_t ldq, const float* datt, int64_t ldo, int64_t B, int32_t T, int32_t H, int32_t dh,
                            float* dqkv, const tgmx_dropout_t* drop, tgmx_stream_t stream);

/* One layer / the whole forward in the saving form: the launches of tgmx_dygformer_layer / tgmx_dygformer_forward in the same order; with
 * dropout off the bits of those.  Layer: x_in -> x_out (may alias); x1, att and qkv are the caller's to keep.  drop: p, seed and the first
 * stream; site s of layer l draws from stream + 4 l + s: 0 attention probabilities [B, H, T, T], 1 the attention block's output [R, D]
 * before the residual, 2 the FFN's hidden activations [R, 4 D], 3 the FFN's output [R, D] before the residual (element = flat index).
 * With dropout sites 1 - 3 are extra launches (tgmx_dropout in place, tgmx_add_cols).
 * Forward: save->counts [2 P L, 2], save->x [(num_layers + 1) R ldx] (layer l's input at l R ldx, the last layer's output last),
 * save->qkv [num_layers R ldq], save->att / save->x1 [num_layers R ldx]; args->ch[], args->mean are kept by the caller too; args->x,
 * x1, att, qkv are not used.  Outside tgmx_mha_small_train_supported: TGMX_E_UNSUPPORTED, nothing launched. */
typedef struct tgmx_dygformer_save {
  int32_t* counts; float *x, *qkv, *att, *x1;
} tgmx_dygformer_save_t;
int tgmx_dygformer_layer_train(const tgmx_dygformer_layer_t* layer, int64_t B, int32_t T, int32_t H, int32_t D, float eps, const float* x_in,
                               float* x_out, float* y, float* x1, float* att, int64_t ldx, float* qkv, int64_t ldq, float* h, int64_t ldh,
                               const tgmx_dropout_t* drop, tgmx_stream_t stream);
int tgmx_dygformer_forward_train(const tgmx_dygformer_fwd_t* args, const tgmx_dygformer_save_t* save, const tgmx_dropout_t* drop,
                                 tgmx_stream_t stream);

/* Patch-mean backward: dx[(2 p + side) Np + t, :D] = dmean[side P + p, :D] / Np. */
int tgmx_dygformer_mean_backward(const float* dmean, int64_t ldm, int64_t P, int32_t Np, int32_t D, float* dx, int64_t ldx, tgmx_stream_t stream);

/* Time-channel backward: from dtime [2 P L, ldt] (the gradient at the Time2Vec features) and the call's ids and times, rows [2 P L, 2 dT]
 * = [ -sin(fma(dt, w, b)) dtime dt | -sin(.) dtime ] (pad slots 0; slot 0: dt = 0); their tgmx_colsum is d time_encoder.w.{weight, bias}. */
int tgmx_dygformer_time_backward(const float* dtime, int64_t ldt, const int32_t* src, const int32_t* dst, const int64_t* edge_time, int64_t P,
                                 const int32_t* nbr_nids, const int64_t* nbr_t, int64_t S, int32_t k, const int32_t* src_rows,
                                 const int32_t* dst_rows, const float* tw, const float* tb, int32_t dT, float* rows, tgmx_stream_t stream);

/* Co-occurrence backward: counts as tgmx_dygformer_cooccurrence wrote them, dfeat [n, ldf] the gradient at the encoded features, n = 2 P L.
 *   onehot [n, up4(L + 1)]: (own == c) + (other == c);  dtable [L + 1, C] = onehot^T dfeat (tgmx_sgemm_tn: a fixed order; pads count 0)
 *   r = relu(w1 c + b1) [L + 1, C];  d W2 = dtable^T r;  d b2 = colsum(dtable);  dh = (dtable W2) [pre > 0] (tgmx_sgemm_nt_ep on w2T [C, C]);
 *   d w1 = colsum(dh o c);  d b1 = colsum(dh)
 * Gradient pointers may be NULL.  workspace: tgmx_dygformer_cooccurrence_backward_workspace_bytes(n, L, C). */
size_t tgmx_dygformer_cooccurrence_backward_workspace_bytes(int64_t n, int32_t L, int32_t C);
int tgmx_dygformer_cooccurrence_backward(const int32_t* counts, const float* dfeat, int64_t ldf, int64_t n, int32_t L, int32_t C,
                                         const float* co_w1, const float* co_b1, const float* co_w2T, float* d_w1, float* d_b1, float* d_w2,
                                         float* d_b2, void* workspace, size_t workspace_bytes, tgmx_stream_t stream);

/* One layer's backward.  x, qkv, att, x1: what tgmx_dygformer_layer_train read and kept; tr: the transposes in_wT [D, 3 D], out_wT [D, D],
 * w1T [D, 4 D], w2T [4 D, D]; g [R, ldx]: the gradient at x_out (clobbered); dx [R, ldx]: the gradient at x_in (NULL: not wanted -- the
 * launches that feed only it are skipped); d: the twelve gradients, each may be NULL.  Order:
 *   y = LN1(x1), a = y w1^T + b1 (recomputed); [p > 0: g3 = tgmx_dropout(g), site 3]; dh = g3 w2; tgmx_mixer_gelu_backward (site 2);
 *   d w2 = g3^T hd, d b2 = colsum(g3), d w1 = da^T y, d b1 = colsum(da); dy = da w1; tgmx_ln_backward -> d ln1; dx1 = du + g;
 *   [p > 0: g1 = tgmx_dropout(dx1), site 1]; d out_w = g1^T att, d out_b = colsum(g1); datt = g1 out_w; tgmx_mha_small_backward (site 0);
 *   y = LN0(x) (recomputed); d in_w = dqkv^T y, d in_b = colsum(dqkv); dy = dqkv in_w; tgmx_ln_backward -> d ln0; dx = du + dx1. */
typedef struct tgmx_dygformer_layer_grad {
  float *ln0_g, *ln0_b, *in_w, *in_b, *out_w, *out_b, *ln1_g, *ln1_b, *w1, *b1, *w2, *b2;
} tgmx_dygformer_layer_grad_t;
typedef struct tgmx_dygformer_layer_tr {
  const float *in_wT, *out_wT, *w1T, *w2T;
} tgmx_dygformer_layer_tr_t;
size_t tgmx_dygformer_layer_backward_workspace_bytes(int64_t B, int32_t T, int32_t D, int64_t ldx, int64_t ldq, int64_t ldh);
int tgmx_dygformer_layer_backward(const tgmx_dygformer_layer_t* layer, const tgmx_dygformer_layer_tr_t* tr,
                                  const tgmx_dygformer_layer_grad_t* d, int64_t B, int32_t T, int32_t H, int32_t D, float eps, const float* x,
                                  const float* qkv, const float* att, const float* x1, int64_t ldx, int64_t ldq, int64_t ldh, float* g,
                                  float* dx, const tgmx_dropout_t* drop, void* workspace, size_t workspace_bytes, tgmx_stream_t stream);

/* The backward of tgmx_dygformer_forward_train as ONE call (tgmx_abi_sizeof(37)), g = dL/dout [2 P, E].  ch / counts / mean / save_*: what
 * that forward wrote; layers / tr: the weights it ran with and their transposes; out_wT [D, E]; proj_w[c] as the forward took them (padded),
 * proj_wT[2], proj_wT[3] [patch ldch[c], C]: the transposes of the time and co-occurrence projections; co_w2T [C, C].  Order:
 *   d out_w = g^T mean, d out_b = colsum(g), dmean = g out_w, tgmx_dygformer_mean_backward; tgmx_dygformer_layer_backward, last layer first;
 *   d proj_w[c] = dtok[:, c C : (c + 1) C]^T ch[c] (one tgmx_sgemm_tn per slot of a patch, written un-padded in the parameter's
 *   [C, patch d] layout), d proj_b[c] = colsum; dtime = dtok_time proj_w[2], tgmx_dygformer_time_backward, two tgmx_colsum;
 *   dfeat = dtok_co proj_w[3], tgmx_dygformer_cooccurrence_backward.
 * Every gradient pointer may be NULL: not wanted, and the launches that feed only it are skipped (the chain stops at the lowest layer
 * with a gradient wanted at or below it).  Written, not accumulated.  No gradient reaches node_x or nbr_x.  No float atomics. */
typedef struct tgmx_dygformer_bwd {
  int64_t P, S; int32_t k, dN, dE, dT, C, patch, heads, E, num_layers; float eps; float drop_p; uint64_t drop_seed, drop_stream;
  const int32_t *src, *dst; const int64_t* edge_time; const int32_t* nbr_nids; const int64_t* nbr_t; const int32_t *src_rows, *dst_rows;
  const float* g; int64_t ldg;
  const float* ch[4]; int64_t ldch[4]; const int32_t* counts; const float* mean;
  const float *save_x, *save_qkv, *save_att, *save_x1; int64_t ldx, ldq, ldh;
  tgmx_dygformer_layer_t layers[TGMX_DYGFORMER_MAX_LAYERS];
  tgmx_dygformer_layer_tr_t tr[TGMX_DYGFORMER_MAX_LAYERS];
  const float *out_wT, *proj_wT[4], *tw, *tb, *co_w1, *co_b1, *co_w2T;
  float *d_tw, *d_tb, *d_co_w1, *d_co_b1, *d_co_w2, *d_co_b2, *d_proj_w[4], *d_proj_b[4], *d_out_w, *d_out_b;
  tgmx_dygformer_layer_grad_t d_layers[TGMX_DYGFORMER_MAX_LAYERS];
  void* workspace; size_t workspace_bytes;
} tgmx_dygformer_bwd_t;
size_t tgmx_dygformer_backward_workspace_bytes(const tgmx_dygformer_bwd_t* args);
int tgmx_dygformer_backward(const tgmx_dygformer_bwd_t* args, tgmx_stream_t stream);

/* ---- TPNet (the reference's tgm/nn/encoder/tpnet.py): temporal walk matrices as random projections, pair features, inference ---- */

/* The num_layer + 1 tables P[0 .. levels) of RandomProjectionModule, each [num_nodes, dim] float32, row-major, contiguous. */
#define TGMX_TPNET_MAX_LEVELS 8
#define TGMX_TPNET_HEAD_EMPTY 0x7f7f7f7f
typedef struct tgmx_tpnet_tables {
  float* P[TGMX_TPNET_MAX_LEVELS];
  int32_t levels, dim;
  int64_t num_nodes;
} tgmx_tpnet_tables_t;

/* RandomProjectionModule.update for one batch of n edges (src, dst int32 [n], time int64 [n]), deterministic, no float atomics:
 * next = time[n - 1]; w_e = exp(-lambda (next - time[e])); every level i >= 1 is scaled by exp(-lambda (next - now) i); then row src[e] of
 * P[i] gains P[i-1][dst[e]] w_e and row dst[e] gains P[i-1][src[e]] w_e, where P[i-1] is the (scaled) table BEFORE this batch adds to
 * it.  A row's contributions are added in the order all sources (e = 0 .. n-1), then all destinations.  Two launches: the first stages
 * every message into msg [(levels - 1) 2 n dim] floats reading the tables only, the second rescales and adds, each element written by
 * one thread.  now: int64 (now_is_f64 = 0) or double on the device; *now_out = next afterwards (may alias now when that is int64).
 * head: [num_nodes] int32 of scratch that holds TGMX_TPNET_HEAD_EMPTY in every entry on entry, and again on exit.  Edges with an endpoint
 * outside [0, num_nodes) contribute nothing.  n = 0: nothing happens.  No device -> host read. */
int tgmx_tpnet_update(const tgmx_tpnet_tables_t* tables, const int32_t* src, const int32_t* dst, const int64_t* time, int64_t n,
                      double lambda, const void* now, int32_t now_is_f64, int64_t* now_out, float* msg, int32_t* head,
                      tgmx_stream_t stream);

/* Pair features of n items (n a multiple of k): item t = q k + j pairs node a[(a_rows ? a_rows[q] : q) k + j] (a row index outside
 * [0, a_num_rows) reads as id -1) with node b0[q mod bmod].  With R_x = the levels rows P[0 .. levels)[x] of a node (a negative id
 * indexes from the end: -1 is the last row), out[t] holds, row-major, concat != 0: the (2 levels)^2 Gram matrix of [R_a; R_b];
 * concat = 0: the levels^2 products R_a R_b^T.  scale != 0: negatives clamped to 0, then log(x + 1).  b1 != NULL: rows [n, 2 n) of out
 * hold the same for b1.  Columns up to ldo zeroed.  levels <= 4, otherwise TGMX_E_UNSUPPORTED.  [n, 2 levels, dim] is never stored. */
int tgmx_tpnet_pair_features(const tgmx_tpnet_tables_t* tables, const int32_t* a, const int32_t* a_rows, int64_t a_num_rows, int32_t k,
                             const int32_t* b0, const int32_t* b1, int64_t bmod, int64_t n, int32_t concat, int32_t scale, float* out,
                             int64_t ldo, tgmx_stream_t stream);

/* TPNet's token matrix, row (q, j) for q < 2 B sequences (sources, then destinations) of k slots read from row rows[q] (NULL: q) of the
 * hop-0 output nbr_* [S, k(, dE)]: [node_x[id] (0 on pad slots) | cos(tw log(edge_time[q mod B] - nbr_t + 1) + tb) (0 on pad slots) |
 * nbr_x as given | pf[row, :pf_dim] | pf[2 B k + row, :pf_dim] | 0 up to ldo].  A row index outside [0, S) reads as all pads, zero
 * edge features. */
int tgmx_tpnet_tokens(const float* node_x, int64_t num_nodes, int32_t dN, const int64_t* edge_time, int64_t B, const int32_t* nbr_nids,
                      const int64_t* nbr_t, const float* nbr_x, int64_t S, int32_t k, int32_t dE, const int32_t* rows, const float* tw,
                      const float* tb, int32_t dT, const float* pf, int64_t ldpf, int32_t pf_dim, float* out, int64_t ldo,
                      tgmx_stream_t stream);

/* tgmx_mixer_token with one correction step on each column's mean (mean += sum(x - mean) / K): the K tokens of an all-pad sequence are
 * identical, and the token LayerNorm of a constant column turns an error d of its mean into d / sqrt(eps) where the exact answer is 0. */
int tgmx_tpnet_token_mix(const float* x, int64_t ldx, int64_t S, int32_t K, int32_t C, const float* tok_g, const float* tok_b,
                         const float* w1, const float* b1, int32_t Ht, const float* w2, const float* b2, const float* ch_g,
                         const float* ch_b, float eps, float* z1, float* y, int64_t ldo, tgmx_stream_t stream);

/* out[q, :C] = mean over the k rows q k .. q k + k - 1 of z. */
int tgmx_tpnet_mean(const float* z, int64_t ldz, int64_t Q, int32_t k, int32_t C, float* out, int64_t ldo, tgmx_stream_t stream);

/* The TPNet inference forward as ONE call: tgmx_tpnet_pair_features for (neighbour, source) and (neighbour, destination), the
 * pair-feature MLP (two GEMMs, ReLU), tgmx_tpnet_tokens, the two projection GEMMs (ReLU between), per layer tgmx_tpnet_token_mix and the
 * channel FFN's two GEMMs, tgmx_tpnet_mean.  tables.levels = 0: no pair-feature columns.  Scratch: feat / pf [4 B k, ldf],
 * feat_h [4 B k, ldfh], x0 [2 B k, ldx0], hp [2 B k, ldhp], z / z1 / y [2 B k, ldz], h [2 B k, ldh]; leading dimensions multiples of 4. */
typedef struct tgmx_tpnet_fwd {
  const float* node_x; int64_t num_nodes;
  const int32_t *src, *dst; const int64_t* edge_time; int64_t B;                   /* the pairs */
  const int32_t* nbr_nids; const int64_t* nbr_t; const float* nbr_x; int64_t S;    /* hop 0: [S, k], [S, k], [S, k, dE] */
  const int32_t* rows;                                                             /* [2 B] rows of hop 0 (sources, destinations), or NULL */
  int32_t k, dN, dE, dT, E, num_layers, rp_concat, rp_scale, rp_out_dim; float eps;
  tgmx_tpnet_tables_t tables;
  const float *rp_w1, *rp_b1, *rp_w2, *rp_b2;                                      /* random_projections.mlp.{0,2} */
  const float *tw, *tb, *proj_w0, *proj_b0, *proj_w2, *proj_b2;                    /* time_encoder.w, projection_layer.{0,2} */
  tgmx_mixer_layer_t layers[TGMX_MIXER_MAX_LAYERS];
  float *feat, *feat_h, *pf, *x0, *hp, *z, *z1, *y, *h; int64_t ldf, ldfh, ldx0, ldhp, ldz, ldh;
  float* out;                                                                      /* [2 B, E] */
} tgmx_tpnet_fwd_t;
int tgmx_tpnet_forward(const tgmx_tpnet_fwd_t* args, tgmx_stream_t stream);

/* ---- TPNet training (csrc/tpnet.hip, csrc/tpnet_bwd.hip; composed by tgm_amd/nn/_tpnet_train.py) ---- */

/* 1 when a sequence's [K, C] tile with token hidden width Ht fits the token forward's LDS (as tgmx_mixer_train_supported) AND
 * tgmx_tpnet_token_backward's: 4 (4 K + 2 Ht) (n + 1) bytes at n = 128, 64 or 32 channels a pass (the widest within 64 KiB), with the
 * partial row of 2 K Ht + 3 K + Ht floats held in registers, at most 24 a thread of that pass.  The host decides the training path with
 * this at forward time. */
int tgmx_tpnet_train_supported(int32_t K, int32_t C, int32_t Ht);

/* tgmx_tpnet_token_mix with the block's two dropout sites, indexed as tgmx_mixer_token_train's; both off: the bits of tgmx_tpnet_token_mix. */
int tgmx_tpnet_token_mix_train(const float* x, int64_t ldx, int64_t S, int32_t K, int32_t C, const float* tok_g, const float* tok_b,
                               const float* w1, const float* b1, int32_t Ht, const float* w2, const float* b2, const float* ch_g,
                               const float* ch_b, float eps, float* z1, float* y, int64_t ldo, const tgmx_dropout_t* drop_hidden,
                               const tgmx_dropout_t* drop_out, tgmx_stream_t stream);

/* tgmx_tpnet_forward in its saving form: the same launches in the same order.  args->feat, feat_h, x0 and hp are the caller's to keep (the
 * backward reads them; pf, y, h, z1 stay scratch); layer l reads its input from save->z + l 2 B k ldz and leaves its token block's output
 * in save->z1 + l 2 B k ldz (args->z receives the last layer's output); save->lg [2 B k] doubles: per token row lg = log(gap + 1), the
 * double the forward feeds the cosine, or -1 on a pad slot (no integer's logarithm).  drop: p, seed and the call's first stream over
 * Q = 2 B sequences, sites as tgmx_graphmixer_forward_train's; NULL or p = 0 = off, and out is then the bits of tgmx_tpnet_forward. */
typedef struct tgmx_tpnet_save {
  float *z, *z1;
  double* lg;
} tgmx_tpnet_save_t;
int tgmx_tpnet_forward_train(const tgmx_tpnet_fwd_t* args, const tgmx_tpnet_save_t* save, const tgmx_dropout_t* drop, tgmx_stream_t stream);

/* dz[q k + j, :C] = g[q, :C] / k: the backward of tgmx_tpnet_mean (TPNet's mean is not masked). */
int tgmx_tpnet_mean_backward(const float* g, int64_t ldg, int64_t Q, int32_t k, int32_t C, float* dz, int64_t ldz, tgmx_stream_t stream);

/* rows [R, 2 dT] = [ -sin(fma(w, lg, b)) d lg | -sin(.) d ] per token row from d = dtime [R, ldt] (the gradient at the time columns of the
 * token matrix) and the forward's lg [R]; a pad row (lg < 0) is 0.  Evaluated in double, rounded once.  tgmx_colsum of the two halves is
 * d time_encoder.w.{weight, bias}. */
int tgmx_tpnet_time_backward(const float* dtime, int64_t ldt, const double* lg, int64_t R, const float* tw, const float* tb, int32_t dT,
                             float* rows, tgmx_stream_t stream);

/* Backward of TPNet's token block (tgmx_tpnet_token_mix_train): tgmx_mixer_token_backward with the forward's refined column mean (a constant
 * column gives var = 0 and xhat = 0 exactly), and with the parameter gradients reduced per sequence instead of written per column: row q of
 * part [Q, ldp] (may be NULL: no parameter gradient wanted; dx has the same bits), ldp >= 2 K Ht + 3 K + Ht, is
 *   [ do^T hd (K x Ht) | da^T xn (Ht x K) | sum do (K) | sum dxn (K) | sum dxn xhat (K) | sum da (Ht) ]
 * summed over the sequence's C columns in a fixed order (channels ascending), i.e. the sequence's share of
 *   [ d ffn.3.weight | d ffn.0.weight | d ffn.3.bias | d token_norm.bias | d token_norm.weight | d ffn.0.bias ];
 * ONE tgmx_colsum over the Q rows gives all six.  Outside tgmx_tpnet_train_supported: TGMX_E_UNSUPPORTED. */
int tgmx_tpnet_token_backward(const float* x, int64_t ldx, const float* dz1, int64_t ldd, int64_t Q, int32_t K, int32_t C, const float* tok_g,
                              const float* tok_b, const float* w1, const float* b1, int32_t Ht, const float* w2, float eps, float* dx,
                              int64_t ldo, float* part, int64_t ldp, const tgmx_dropout_t* drop_hidden, const tgmx_dropout_t* drop_out,
                              tgmx_stream_t stream);

/* The backward of tgmx_tpnet_forward_train as ONE call (tgmx_abi_sizeof(38)), g = dL/d[z_src; z_dst] [2 B, E].  It reads what that forward
 * kept (feat, feat_h, x0, hp, save_z, save_z1, lg) and packed copies of the weights (one tgmx_pack2d) -- none of the caller's input tensors:
 *   proj_w2T [2 E, E]; w0T_time [dT, 2 E], w0T_pair0 / w0T_pair1 [od, 2 E]: the transposed column slices of proj_w0 that somebody reads;
 *   rp_w2T [4 od, od]; per layer ch_w1T [E, Hc], ch_w2T [Hc, E].
 * Every gradient pointer may be NULL: not wanted, and the launches that feed only it are skipped; gradients are written, not accumulated,
 * in the parameters' own layouts.  d_tok[l]: the six token-block gradients of layer l as ONE buffer of 2 K Ht + 3 K + Ht floats in
 * tgmx_tpnet_token_backward's column order (d_layers[l].tok_* are not read).  No float atomics: two runs give the same bits.  Order:
 *   tgmx_tpnet_mean_backward -> gz;  per layer, last first: the channel block (tgmx_graphmixer_backward's launches), then
 *   tgmx_tpnet_token_backward -> gz, part and one tgmx_colsum(part) -> d_tok[l];
 *   d proj_w2 = gz^T hp, d proj_b2 = colsum(gz), dhp = gz W2 (tgmx_sgemm_nt_ep on proj_w2T), tgmx_relu_mask by hp, d proj_w0 = dhp^T x0,
 *   d proj_b0 = colsum(dhp); dtime = dhp w0T_time^T, tgmx_tpnet_time_backward, two tgmx_colsum -> d_tw, d_tb;
 *   dpf[0:R] = dhp w0T_pair0^T, dpf[R:2R] = dhp w0T_pair1^T; d rp_w2 = dpf^T feat_h, d rp_b2 = colsum(dpf), dfh = dpf W2 (rp_w2T),
 *   tgmx_relu_mask by feat_h, d rp_w1 = dfh^T feat, d rp_b1 = colsum(dfh).
 * The chain stops at the lowest stage that still has a gradient wanted at or below it. */
typedef struct tgmx_tpnet_bwd {
  int64_t B; int32_t k, dN, dE, dT, E, od, num_layers; float eps; float drop_p; uint64_t drop_seed, drop_stream;
  const float* g; int64_t ldg;
  const float *feat, *feat_h, *x0, *hp, *save_z, *save_z1; const double* lg; int64_t ldf, ldfh, ldx0, ldhp, ldz, ldh;
  const float *tw, *tb;
  tgmx_mixer_layer_t layers[TGMX_MIXER_MAX_LAYERS];
  const float* ch_w1T[TGMX_MIXER_MAX_LAYERS]; const float* ch_w2T[TGMX_MIXER_MAX_LAYERS];
  const float *proj_w2T, *w0T_time, *w0T_pair0, *w0T_pair1, *rp_w2T;
  float *d_tw, *d_tb, *d_proj_w0, *d_proj_b0, *d_proj_w2, *d_proj_b2, *d_rp_w1, *d_rp_b1, *d_rp_w2, *d_rp_b2;
  tgmx_mixer_layer_grad_t d_layers[TGMX_MIXER_MAX_LAYERS];
  float* d_tok[TGMX_MIXER_MAX_LAYERS];
  void* workspace; size_t workspace_bytes;
} tgmx_tpnet_bwd_t;
size_t tgmx_tpnet_backward_workspace_bytes(const tgmx_tpnet_bwd_t* args);
int tgmx_tpnet_backward(const tgmx_tpnet_bwd_t* args, tgmx_stream_t stream);

/* ---- NCNPredictor (the reference's tgm/nn/decoder/ncnpred.py): the common-neighbour decoder of TNCN, forward ---- */

/* The symmetric adjacency of edge_index [2, E] (int64 when is64, else int32; row 1 starts row_stride entries after row 0) over N local
 * node ids, as sorted rows: A[a, b] = how often (a, b) or (b, a) occurs, so a self-loop counts twice.  indptr [N + 1]; cols [2 E] holds
 * every row's neighbour ids ascending, an id repeated as often as it occurs.  One radix sort of the 2 E (row, col) keys: the result does
 * not depend on scheduling, and a row may be as long as 2 E.  An edge with an endpoint outside [0, N) is left out.  2 E < 2^31.
 * workspace: tgmx_ncn_adj_workspace_bytes(E) bytes (0: E out of range). */
size_t tgmx_ncn_adj_workspace_bytes(int64_t E);
int tgmx_ncn_adj_build(const void* edge_index, int32_t is64, int64_t row_stride, int64_t E, int64_t N, int32_t* indptr, int32_t* cols,
                       void* workspace, size_t workspace_bytes, tgmx_stream_t stream);

/* xs [B, ldxs] for the pairs tar [2, B] (int64 / int32, row stride tar_stride), k = 2 or 4 blocks of C columns:
 *   x[i] * x[j] | (k = 4: A[j, i] W[r, i] x[i] | A[i, j] W[r, j] x[j]) | sum over n of A[i, n] A[j, n] W[r, n] x[n]   (ascending n)
 * with W[r, n] = exp(-(float32(edge_time[r] - last_update[n]) / 10000)), or 1 when last_update and edge_time are NULL.  last [2 N] int32
 * of scratch: a pair keeps its blocks after the first only where r is the LAST position of tar[0][r] in tar[0] and of tar[1][r] in tar[1]
 * (the reference's CPU behaviour); last = NULL: every pair keeps them.  A pair with a target outside [0, N) gets a zero row.  Columns up
 * to ldxs zeroed.  One wave per pair, fixed summation order, no float atomics. */
int tgmx_ncn_cn_emb(const float* x, int64_t N, int32_t C, int32_t k, const int32_t* indptr, const int32_t* cols, const void* tar,
                    int32_t tar_is64, int64_t tar_stride, int64_t B, const int64_t* last_update, const int64_t* edge_time, int32_t* last,
                    float* xs, int64_t ldxs, tgmx_stream_t stream);

/* The NCNPredictor inference forward as ONE call: tgmx_ncn_adj_build (skipped when have_adj: indptr / cols hold a prepared adjacency),
 * tgmx_ncn_cn_emb, out = W2 relu(W1 xs + b1) + b2 (two GEMMs).  Scratch: indptr [N + 1], cols [2 E], adj_ws, last [2 N], xs [B, ldxs],
 * h [B, ldh]; ldxs and ldh multiples of 4. */
typedef struct tgmx_ncn_fwd {
  const float* x; int64_t N;
  int32_t C, k, H, out_ch, decay, dup_all;                      /* dup_all: every duplicate target keeps its adjacency row */
  const void* edge_index; int64_t ei_stride, E; int32_t ei_is64, have_adj;
  const void* tar; int64_t tar_stride, B; int32_t tar_is64, reserved_;
  const int64_t *last_update, *edge_time;                       /* [N], [B]; read when decay */
  const float *w1, *b1, *w2, *b2;                               /* xsmlp.{0,2} */
  int32_t *indptr, *cols; void* adj_ws; size_t adj_ws_bytes;
  int32_t* last;
  float *xs, *h; int64_t ldxs, ldh;
  float* out;                                                   /* [B, out_ch] */
} tgmx_ncn_fwd_t;
int tgmx_ncn_forward(const tgmx_ncn_fwd_t* args, tgmx_stream_t stream);

/* ---- NCNPredictor at k = 8 (csrc/ncn8.hip): the two-hop common-neighbour blocks.  tgmx_ncn_cn_emb / tgmx_ncn_forward and the backward
 * entries below keep refusing k = 8; these three take it.  With A2 = A A, K3 = A2 A, u = -A[i, j], R = A[t], S = A2[t] for the pair (i, j):
 *   c01[i] = A[j, i]   c10[j] = A[i, j]   c11 = R_i o R_j   sp = c11 A
 *   c12 = R_i o S_j + R_i o R_i u      c21 = S_i o R_j + R_j o R_j u
 *   c22 = S_i o S_j + ([R_i > 0] K3[i, i] + [R_j > 0] K3[j, j] - c11) u + sp
 *   c12, c21, c22: columns i and j set to 0, then c22 = max(c22, 0)
 *   xs[r] = x[i] * x[j] | (c01 o W) x | (c10 o W) x | (c11 o W) x | (c12 o W) x | (c21 o W) x | (c22 o W) x | sp x       (8 C columns)
 * Every coefficient is an exact integer (int32 count rows, int64 products), W (tgmx_ncn_cn_emb's float32 argument, the exponential in
 * float64) multiplies only non-zero counts, the sums run over ascending n in float64 and are rounded once: no float atomics, two runs give
 * the same bits.  last, the zero row of a pair
 * with a target outside [0, N) and the columns up to ldxs: as tgmx_ncn_cn_emb.  One workgroup per pair; the count rows live in LDS while
 * N <= tgmx_ncn8_lds_max_nodes(), else in the workspace (5 N int32 per resident workgroup, zeroed once per call).
 * workspace: tgmx_ncn8_workspace_bytes(N, B) bytes, host arithmetic only (0: a size out of range).  force_workspace != 0 (tests): the
 * workspace form whatever N; it needs what tgmx_ncn8_workspace_bytes gives for any N' > max(N, tgmx_ncn8_lds_max_nodes()). */
int32_t tgmx_ncn8_lds_max_nodes(void);
size_t tgmx_ncn8_workspace_bytes(int64_t N, int64_t B);
int tgmx_ncn8_cn_emb(const float* x, int64_t N, int32_t C, const int32_t* indptr, const int32_t* cols, const void* tar, int32_t tar_is64,
                     int64_t tar_stride, int64_t B, const int64_t* last_update, const int64_t* edge_time, int32_t* last, float* xs,
                     int64_t ldxs, void* workspace, size_t workspace_bytes, int32_t force_workspace, tgmx_stream_t stream);
/* The k = 8 inference forward as ONE call: tgmx_ncn_forward's argument block (k = 8, ldxs >= 8 C) and steps, with tgmx_ncn8_cn_emb; the
 * two Linear layers (8 C integer-weighted inputs, hidden units in the hundreds) run as one float64 kernel, a workgroup per pair, the hidden
 * row unrounded in LDS, out rounded once (h receives the float32 copy); H > 8192 is refused (TGMX_E_INVALID). */
int tgmx_ncn8_forward(const tgmx_ncn_fwd_t* args, void* workspace, size_t workspace_bytes, tgmx_stream_t stream);

/* ---- NCNPredictor training (csrc/ncn_bwd.hip): the backward of the common-neighbour stage, and the whole backward as ONE call.  No float
 * atomics anywhere: every sum has one fixed order, two runs give the same bits.  Nothing is read back to the host. ---- */

/* dx [N, C] (contiguous; EVERY row is written, zeros where nothing contributes) from dxs [B, lddxs], the gradient of tgmx_ncn_cn_emb's xs,
 * with g0 .. g3 the C-wide column blocks of dxs[r] (g_cn the last of the k).  Node n receives, in this order:
 *   (1) every in-range pair r with tar_i[r] = n, ascending r:  g0[r] * x[tar_j[r]]; then, k = 4, r active, m = A[i, j] > 0:  m W[r, i] g1[r]
 *   (2) every in-range pair r with tar_j[r] = n, ascending r:  g0[r] * x[tar_i[r]]; then, k = 4, r active, m > 0:            m W[r, j] g2[r]
 *   (3) every active pair r with A[n, i_r] > 0 and A[n, j_r] > 0, ascending (i_r, r):  A[n, i_r] A[n, j_r] W[r, n] g_cn[r]
 * A pair with i = j contributes through (1) and (2).  Active is the forward's rule: last = NULL: every in-range pair; else last [2 N] as
 * tgmx_ncn_cn_emb left it.  A pair with a target outside [0, N) contributes nothing and is never dereferenced.  W and A are the forward's,
 * bit for bit (last_update / edge_time NULL: W = 1).  indptr / cols: the adjacency of tgmx_ncn_adj_build over E edges.
 * The pairs are read through two inverted indexes (by tar_i, by tar_j: ONE radix sort of 2 B keys); a wave per node keeps 256 channels in
 * registers and stores once.  A row of more than 512 entries leaves term (3) to two further launches, issued whenever 2 E > 512: a wave per
 * 256-entry chunk of the entry array, then the row's chunk sums in ascending chunk order onto its terms (1) and (2).  No degree bound.
 * 2 N, 2 E, 2 B < 2^31.  workspace: tgmx_ncn_dx_workspace_bytes(N, E, B, C) bytes, host arithmetic only (0: a size out of range). */
size_t tgmx_ncn_dx_workspace_bytes(int64_t N, int64_t E, int64_t B, int32_t C);
int tgmx_ncn_dx(const float* x, int64_t N, int32_t C, int32_t k, const int32_t* indptr, const int32_t* cols, int64_t E, const void* tar,
                int32_t tar_is64, int64_t tar_stride, int64_t B, const int64_t* last_update, const int64_t* edge_time, const int32_t* last,
                const float* dxs, int64_t lddxs, float* dx, void* workspace, size_t workspace_bytes, tgmx_stream_t stream);

/* The backward's argument block (tgmx_abi_sizeof(33)).  fwd: the block tgmx_ncn_forward ran with -- the inputs, the weights where the
 * parameters are, and what that call wrote into buffers of ITS OWN: xs, h (post-ReLU), last, indptr, cols (or the prepared adjacency);
 * edge_index, adj_ws and out are not read.  dout [B, out_ch] with leading dimension lddout.  Every gradient pointer may be NULL: that
 * gradient, and every launch that only feeds it, is skipped.  d_x [N, C], d_w1 [H, k C], d_b1 [H], d_w2 [out_ch, H], d_b2 [out_ch], all
 * contiguous, in the parameters' own layouts.  last_update / edge_time get no gradient (W depends on integers only).
 * Order: the weights transposed (one tgmx_pack2d) -> the last layer (tgmx_decoder_tail_bwd with the ReLU mask read from h where
 * out_ch <= 16 and W2 fits 48 KB; else tgmx_sgemm_tn, tgmx_colsum, tgmx_sgemm_nt, tgmx_relu_mask) -> d_w1 = dpre^T xs (tgmx_sgemm_tn),
 * d_b1 (tgmx_colsum) -> dxs = dpre W1 (tgmx_sgemm_nt; only for d_x) -> tgmx_ncn_dx.  B = 0: the gradients asked for are zeroed.
 * workspace: tgmx_ncn_backward_workspace_bytes() (host only; 0 for sizes out of range, e.g. 2 E >= 2^31). */
typedef struct tgmx_ncn_bwd {
  tgmx_ncn_fwd_t fwd;
  const float* dout; int64_t lddout;
  float *d_x, *d_w1, *d_b1, *d_w2, *d_b2;
  void* workspace; size_t workspace_bytes;
} tgmx_ncn_bwd_t;
size_t tgmx_ncn_backward_workspace_bytes(const tgmx_ncn_bwd_t* args);
int tgmx_ncn_backward(const tgmx_ncn_bwd_t* args, tgmx_stream_t stream);

/* ---- EdgeBankPredictor (the reference's tgm/nn/modules/edgebank.py): the edge memory as a device hash table ---- */

/* table: capacity slots of 16 bytes {uint64 key = src << 32 | dst, int64 ts}, open addressing with linear probing from
 * splitmix64(key) & (capacity - 1); capacity a power of two; an empty slot has key = all ones (and the caller fills a new table so).  stamp
 * [capacity] int64, zeroed with a new table: the arrival number of the event whose ts the slot holds (only the update reads or writes it).
 * state: tgmx_edgebank_state_bytes() bytes {int64 window_end, int64 window_size (unlimited mode), float32 window_size (fixed mode), pad};
 * the window start is window_end - window_size in int64, or (float)window_end - window_size in float32 when fixed.  status: one int32 of
 * sticky bits: 1 = an id outside [0, 2^31) was offered or queried (it contributes nothing / answers 0), 2 = a probe ran through the whole
 * table (the caller let it fill: capacity must stay >= 2 x the entries). */
typedef struct tgmx_edgebank {
  void* table; int64_t* stamp; int64_t capacity;
  void* state;
  int32_t fixed, reserved_;                                     /* fixed: memory_mode == 'fixed' */
  double pos_prob;                                              /* what a hit answers, cast to the output dtype as torch casts it */
  int64_t arrivals;                                             /* events offered to tgmx_edgebank_update before this call */
  int32_t* status;
} tgmx_edgebank_t;
size_t tgmx_edgebank_state_bytes(void);

/* One batch of the reference's update(): window_end = max(window_end, max ts); then every event with ts >= the new window start (fixed
 * mode: both sides rounded to float32) stores its ts under (src, dst), and of several events of one pair the LAST in arrival order (position
 * in the call, then call order) is the one kept, whatever its ts.  ids / ts int64 where the *_is64 flag is set, else int32.  n <= 1024 is
 * one workgroup and one launch, more is three launches.  No float atomics, nothing depends on scheduling but the slot positions. */
int tgmx_edgebank_update(const tgmx_edgebank_t* eb, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const void* ts,
                         int32_t ts_is64, int64_t n, tgmx_stream_t stream);

/* out[i] = pos_prob where the pair is stored (fixed mode: and its int64 ts >= the float32 window start, compared exactly), else 0; one lane
 * per answer.  neg == NULL: `total` = B pairs (src[i], dst[i]).  Otherwise row b answers (src[b], dst[b]) and then (src[b], neg[b][m]): neg
 * is [B, M] with neg_off == NULL (total = B (M + 1)), or the rows laid end to end with neg_off [B + 1] their int64 offsets (total = B +
 * neg_off[B]); row b's answers start at neg_off[b] + b.  out_dtype: 0 int32, 1 int64, 2 float32, 3 float64. */
int tgmx_edgebank_query(const tgmx_edgebank_t* eb, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const void* neg,
                        int32_t neg_is64, const int64_t* neg_off, int64_t M, int64_t B, int64_t total, void* out, int32_t out_dtype,
                        tgmx_stream_t stream);

/* Moves the entries of `from` into `to` (a new, empty table of at least twice the capacity); in fixed mode entries whose ts has left the
 * window (the update's test, against from->state) are dropped, as the reference's _clean_up drops them.  *kept (device) = entries moved. */
int tgmx_edgebank_rehash(const tgmx_edgebank_t* from, const tgmx_edgebank_t* to, int64_t* kept, tgmx_stream_t stream);

/* ---- tCoMemPredictor (the reference's tgm/nn/modules/t_comem.py): recent-event rings, popularity and pair counts on the device ---- */

/* ring: [num_nodes, k] entries of 8 bytes {float32 ts, int32 dst}, the k most recent events with the node as source; the caller fills a new
 * ring with {-inf, -1}.  pos, len, popularity: [num_nodes] int32, zeroed: where the node's next event goes, how many entries are filled
 * (<= k), how often the node was a destination.  table: the pair counts, slots as tgmx_edgebank_t's with key = min(s, d) << 32 | max(s, d)
 * and value = the count (a self-loop counts 2: the reference increments [s][d] and [d][s]); filled {all ones, 0} when new.  state:
 * tgmx_tcomem_state_bytes() bytes {int64 end = the largest timestamp seen, float32 size = the window size, pad}; the window is
 * [f32(f32(end) - size), f32(end)].  status: one int32 of sticky bits: 1 = an id outside [0, 2^31), 2 = a probe ran through the whole table
 * (capacity must stay >= 2 x the pairs), 4 = a source >= num_nodes, 8 = an update's destination >= num_nodes.  A flagged event contributes
 * nothing, a flagged query answers 0. */
typedef struct tgmx_tcomem {
  void* ring; int32_t *pos, *len, *popularity;
  void* table; int64_t capacity;
  void* state;
  int64_t num_nodes; int32_t k, reserved_;
  double co_occurrence_weight;
  int32_t* status;
} tgmx_tcomem_t;
size_t tgmx_tcomem_state_bytes(void);

/* One batch of the reference's update(), in event order: end = max(end, max ts); per event the pair's count += 1 (2 for a self-loop),
 * popularity[dst] += 1, and the event {f32(ts), dst} goes to ring[src][pos], pos advancing modulo k and len saturating at k, whatever the
 * timestamp.  ids / ts int64 where the *_is64 flag is set, else int32.  One workgroup and one launch per 1024 events, in arrival order.
 * Integer atomics only; nothing depends on scheduling but the slot positions in the table. */
int tgmx_tcomem_update(const tgmx_tcomem_t* tc, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const void* ts,
                       int32_t ts_is64, int64_t n, tgmx_stream_t stream);

/* out (float32) = base(src) + the co-occurrence term.  base(s) = sum over ring entries i < len[s] with start <= ts <= f32(end) of
 * exp(-(f32(end) - ts) / size) * sigmoid(popularity[dst]) in float32, the same bits for a source wherever it appears.  With c the pair's
 * count and t = co_occurrence_weight * (c / (1 + c)) in double, query_dtype (the dtype of the ids the reference would have been handed:
 * 0 int32, 1 int64, 2 float32, 3 float64) decides the term as the reference's zeros_like(query_src) does: 0 / 1 add nothing, 2 adds
 * (float)t in float32, 3 adds t in double and rounds the sum.  Rows as in tgmx_edgebank_query, one wave per row: neg == NULL: `total` = B
 * pairs; else row b answers (src[b], dst[b]) and then (src[b], neg[b][m]), neg [B, M] (total = B (M + 1)) or ragged through neg_off [B + 1]
 * (total = B + neg_off[B]; row b's answers start at neg_off[b] + b). */
int tgmx_tcomem_query(const tgmx_tcomem_t* tc, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const void* neg,
                      int32_t neg_is64, const int64_t* neg_off, int64_t M, int64_t B, int64_t total, float* out, int32_t query_dtype,
                      tgmx_stream_t stream);

/* Moves the pair counts of `from` into `to` (a new, empty table of at least twice the capacity).  *kept (device) = pairs moved. */
int tgmx_tcomem_rehash(const tgmx_tcomem_t* from, const tgmx_tcomem_t* to, int64_t* kept, tgmx_stream_t stream);

/* ---- CTAN (the reference's tgm/nn/encoder/ctan.py): memory update, wide-head attention, the encoder's forward and its backward ---- */

/* CTANMemory.update_state (ctan.py:128-147) with LastAggregator: over the positions p in [0, 2B) of cat[src, pos_dst] (time t[p mod B]),
 * a node's memory row becomes row p* of cat[src_emb, pos_dst_emb], p* = the LOWEST p among the node's positions with the largest
 * float32(t) (the reference's argmax over float scores), and its last_update the exact int64 maximum of its times -- plain overwrites, no
 * maximum against the old state.  src_emb has rows_src >= B rows, [*, M]; row p >= rows_src is pos_dst_emb's row p - rows_src (the caller
 * checks that the two hold 2B rows).  ids int64 where the *_is64 flag is set, else int32.  scratch_key [num_nodes] 8-byte words, all
 * ZERO, and scratch_tmax [num_nodes] int64, all INT64_MIN, on entry; both are left so (the caller keeps them between calls).  Two
 * launches, integer atomic maxima only: the same bits on every run.  An id outside [0, num_nodes) is skipped and sets bit 1 of *status. */
int tgmx_ctan_memory_update(const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const int64_t* t, int64_t B,
                            const float* src_emb, const float* dst_emb, int64_t rows_src, int32_t M, int64_t num_nodes, float* memory,
                            int64_t* last_update, void* scratch_key, int64_t* scratch_tmax, int32_t* status, tgmx_stream_t stream);

/* The attention of TransformerConv(heads = 1, root_weight = False) (third-party definition, PyG 2.6.1) with AntiSymmetricConv's update as
 * its epilogue.  Arguments as tgmx_tconv_attend's with H = 1; `order` must hold every segment in ascending edge id (tgmx_segment_sort),
 * src[e] in [0, U).  With phi_i = sum_j softmax_j(q_i.(k_j + e_ij) scale) (v_j + e_ij), 0 for a target without incoming edges:
 *   mode 0: h4 += phi;   mode 1: x <- x + epsilon tanh(h4 + phi);   mode 2: out = tanh(x + epsilon tanh(h4 + phi)),
 * every one of the U rows included.  C <= 256: one wave covers a row (a lane owns ceil(C / 64) consecutive columns), edges in blocks of
 * four requested ahead, long segments over four waves merged in wave order -- deterministic.  Wider: tgmx_tconv_attend's walk, then
 * the epilogue as a launch of its own. */
int tgmx_ctan_attend(const float* q, const float* k, const float* v, const float* eproj, const int64_t* order, const int64_t* src,
                     const int64_t* seg_lo, const int64_t* seg_hi, int64_t U, int32_t C, float scale, float* h4, float* x, float* out,
                     float epsilon, int32_t mode, tgmx_stream_t stream);

/* CTAN.forward (ctan.py:53-79; AntiSymmetricConv and TransformerConv from their PyG 2.6.1 definitions) as ONE call, inference only:
 *   x = node_x W_x^T + b_x;  once: edge_attr[e] = [msg[e] | cos(rel_e tw + tb)], rel_e = (float(|last_update[src[e]] - t[e]|) - mean_delta_t)
 *   / std_delta_t in float32, eproj = edge_attr W_edge^T, the edges grouped by tgt (tgmx_segment_sort);  num_iters times: qkvs = x W4^T + b4
 *   (W4 = [W_query, W_key, W_value, A], A = W - W^T - gamma I; b4 = [b_query, b_key, b_value, bias]: one batched GEMM), then
 *   tgmx_ctan_attend in mode 1 (mode 2 on the last iteration, into out).
 * Every buffer is the caller's.  src / tgt out of [0, U) are clamped and raise TGMX_ST_EDGE_RANGE in *status.
 * x_save (appended; NULL = the behaviour above, x updated in place): the saving forward of the training path.  [max(num_iters, 1), U, M]:
 * slot 0 receives enc_x(node_x), iteration `it` reads slot `it` and writes slot `it + 1` (the last one writes `out` only); `x` is then
 * not touched and may be NULL.  The same kernels in the same order: `out` has the bits of the call without x_save. */
typedef struct tgmx_ctan_fwd {
  const float* node_x; int64_t U; int32_t in_ch, M;    /* [U, in_ch], in_ch = M + node_dim */
  const int64_t* last_update;                          /* [U] */
  const int64_t* src; const int64_t* tgt; const int64_t* t; const float* msg; int64_t E; int32_t D, T;
  const float* tw; const float* tb;                    /* [T], [T] */
  const float* W_x; const float* b_x;                  /* [M, in_ch], [M] */
  const float* W4; const float* b4; const float* W_edge; /* [4, M, M], [4, M], [M, D + T] */
  int32_t num_iters; float epsilon, mean_delta_t, std_delta_t;
  float* edge_attr; float* eproj; float* x; float* qkvs; /* [E, D + T], [E, M], [U, M], [4, U, M] */
  int64_t* src_ok; int64_t* order; int64_t* seg_lo; int64_t* seg_hi; /* [E], [E], [U], [U] */
  void* sort_ws; size_t sort_ws_bytes; int32_t* status;
  float* out;                                          /* [U, M] */
  float* x_save;                                       /* [max(num_iters, 1), U, M] or NULL */
} tgmx_ctan_fwd_t;
int tgmx_ctan_forward(const tgmx_ctan_fwd_t* args, tgmx_stream_t stream);

/* ---- CTAN training: the backward of tgmx_ctan_forward (csrc/ctan_bwd.hip).  No float atomics, every sum in a fixed order. ---- */

/* The final tanh: gx[r, c] = g[r, c] (1 - out[r, c]^2);  g [U, M] with leading dimension ldg, out and gx [U, M] dense. */
int tgmx_ctan_out_backward(const float* g, int64_t ldg, const float* out, int64_t U, int32_t M, float* gx, tgmx_stream_t stream);

/* The target pass of one AntiSymmetricConv iteration, C <= 256, one workgroup per target i (lane ownership, blocks of four and the four-wave
 * split above 16 edges as tgmx_ctan_attend).  q, k, v, h4 [U, C], eproj, order, src, seg_lo, seg_hi: what tgmx_ctan_attend read (h4 = x A^T
 * + bias, before the attention); seg_lo NULL: no edges at all.  Walk 1 recomputes the row's softmax state (m, l) and phi as the forward
 * does; then, with z_i = h4_i + phi_i,
 *   dz_i = epsilon gx_i (1 - tanh^2 z_i),   delta_i = dz_i . phi_i,
 * and walk 2, per incoming edge e (source j) in ascending edge id:
 *   alpha_e = exp(scale q_i.(k_j + ep_e) - m) / l,   dalpha_e = dz_i . (v_j + ep_e),   s_e = scale alpha_e (dalpha_e - delta_i),
 *   dq_i = sum_e s_e (k_j + ep_e)   (merged in wave order),
 *   d_eproj[e] (+)= s_e q_i + alpha_e dz_i   (d_eproj NULL: not wanted; accumulate != 0 adds to the row: every edge has one target, so
 *   its owner does a plain read-modify-write),   alpha[e], s[e] and etgt[e] = i.
 * d4 [U, 4C]: dq_i goes to columns [0, C), dz_i to [3C, 4C) (the source pass fills the two blocks between).  A target without incoming
 * edges gets dq = 0 and dz from z = h4. */
int tgmx_ctan_attend_backward(const float* q, const float* k, const float* v, const float* h4, const float* eproj, const int64_t* order,
                              const int64_t* src, const int64_t* seg_lo, const int64_t* seg_hi, int64_t U, int32_t C, float scale, float epsilon,
                              const float* gx, float* d4, float* alpha, float* s, int32_t* etgt, float* d_eproj, int32_t accumulate,
                              tgmx_stream_t stream);

/* The source pass: one workgroup per source j over the edges grouped by source (order_s, sseg_lo, sseg_hi: tgmx_segment_sort on src, each
 * segment in ascending edge id):
 *   dk_j = sum_e s[e] q[etgt[e]],   dv_j = sum_e alpha[e] dz[etgt[e]]     (dz = d4's columns [3C, 4C)),
 * written to d4's columns [C, 2C) and [2C, 3C); zero rows for a source without outgoing edges.  More than 16 edges: split over the four
 * waves and merged in wave order.  sseg_lo NULL: no edges.  This replaces the float atomics of tgmx_tconv_attend_backward. */
int tgmx_ctan_source_backward(const float* q, float* d4, const int64_t* order_s, const int32_t* etgt, const int64_t* sseg_lo,
                              const int64_t* sseg_hi, const float* alpha, const float* s, int64_t U, int32_t C, tgmx_stream_t stream);

/* The time encoder's backward, per edge: rel_e = (float(|last_update[src[e]] - t[e]|) - mean) / std in float32 as the forward computes it,
 *   gs = -sin(rel_e tw[c] + tb[c]) d_attr[e, c];   part[e, c] = gs rel_e  (d tw),   part[e, T + c] = gs  (d tb);
 * d_attr [E, T] with leading dimension ldd (the gradient at the time columns of edge_attr), part [E, 2T]; sum the rows with tgmx_colsum.
 * src[e] in [0, U) (the forward's src_ok). */
int tgmx_ctan_edge_attr_backward(const int64_t* last_update, const int64_t* src, const int64_t* t, const float* tw, const float* tb,
                                 const float* d_attr, int64_t ldd, int32_t T, int64_t E, float mean, float std, float* part,
                                 tgmx_stream_t stream);

/* A = W - W^T - gamma I:  dW[r, c] = dA[r, c] - dA[c, r];  both [M, M] dense, dW must not alias dA. */
int tgmx_ctan_antisym_grad(const float* dA, int32_t M, float* dW, tgmx_stream_t stream);

/* The backward of tgmx_ctan_forward as ONE call (tgmx_abi_sizeof(35)), M <= 256.  x_save / out / edge_attr / eproj / src_ok / order /
 * seg_lo / seg_hi: what the saving forward wrote (buffers of that call).  With g = dL/dout:
 *   gx = g (1 - out^2);  the edges grouped by source once (tgmx_segment_sort on src_ok);
 *   it = num_iters - 1 .. 0:  qkvs = x_it W4^T + b4 (the forward's GEMM) -> tgmx_ctan_attend_backward -> tgmx_ctan_source_backward ->
 *     d_W4[b] (+)= d_b^T x_it (one batched tgmx_sgemm_tn), d_b4 (+)= colsum(d4) -> gx <- gx + d4 W4T^T (tgmx_sgemm_nt_ep, res = gx);
 *   d_W = d_W4[3] - d_W4[3]^T;  d_Wx = gx^T node_x, d_bx = colsum(gx), d_node_x = gx WxT^T;  d_Wedge = d_eproj^T edge_attr;
 *   d_time = [d tw | d tb] = colsum(tgmx_ctan_edge_attr_backward(d_eproj WeT^T)).
 * W4T [M, 4M] = W4 viewed as [4M, M], transposed;  WxT [in_ch, M] = W_x^T (only for d_node_x);  WeT [T, M] = W_edge[:, D:]^T (only for
 * d_time).  A NULL output is not wanted and its work is skipped (d_W needs d_W4).  num_iters = 0 or E = 0: the gradients that no path
 * reaches are zeroed.  U = 0 returns at once. */
typedef struct tgmx_ctan_bwd {
  int64_t U, E; int32_t in_ch, M, D, T, num_iters; float epsilon, mean_delta_t, std_delta_t;
  const float* g; int64_t ldg;                         /* dL/dout [U, M] */
  const float* out; const float* x_save;               /* [U, M], [max(num_iters, 1), U, M] */
  const float* node_x;                                 /* [U, in_ch] (d_Wx) */
  const int64_t* last_update; const int64_t* t;        /* [U], [E] (d_time) */
  const float* tw; const float* tb;                    /* [T], [T] (d_time) */
  const float* W4; const float* b4;                    /* [4, M, M], [4, M]: the forward's */
  const float* W4T; const float* WxT; const float* WeT; /* [M, 4M], [in_ch, M], [T, M] */
  const float* edge_attr; const float* eproj;          /* [E, D + T], [E, M] */
  const int64_t* src_ok; const int64_t* order; const int64_t* seg_lo; const int64_t* seg_hi;
  float* d_W4; float* d_b4; float* d_W;                /* [4, M, M], [4, M], [M, M] */
  float* d_Wx; float* d_bx; float* d_node_x;           /* [M, in_ch], [M], [U, in_ch] */
  float* d_Wedge; float* d_time;                       /* [M, D + T], [2T] */
  void* workspace; size_t workspace_bytes;
} tgmx_ctan_bwd_t;
size_t tgmx_ctan_backward_workspace_bytes(const tgmx_ctan_bwd_t* args);
int tgmx_ctan_backward(const tgmx_ctan_bwd_t* args, tgmx_stream_t stream);

/* ---- ChebConv / GCLSTM (the reference's tgm/nn/encoder/gclstm.py; ChebConv from its published PyG definition): the scaled Laplacian of a
 * snapshot as a CSR by destination, a gather SpMM over it, and the cell's inference forward as one call ---- */

#define TGMX_CHEB_NORM_NONE 0
#define TGMX_CHEB_NORM_SYM 1
#define TGMX_CHEB_NORM_RW 2

/* Bytes of workspace tgmx_cheb_laplacian needs for E edges over N nodes (0: sizes out of range). */
size_t tgmx_cheb_workspace_bytes(int64_t E, int64_t N);

/* L_hat = 2 L / lambda_max - I of the graph (src[e] -> dst[e], weight w[e] or 1) as rows BY DESTINATION: indptr [N + 1], cols [E] (the
 * sources, ascending within a row, duplicates kept in edge order), vals [E], and the diagonal diag [N].  Self loops are dropped; the degree
 * is taken over the SOURCE index; normalization NONE: m_e = -w, d_i = deg_i;  SYM: m_e = -deg[src]^-1/2 w deg[dst]^-1/2, d_i = 1;
 * RW: m_e = -w / deg[src], d_i = 1 (an infinite factor counts as 0);  vals = 2 m_e / lambda_max (infinite -> 0), diag = 2 d_i / lambda_max - 1.
 * lambda_max is read from lambda_ptr (device, one float) when that is non-NULL.  ids int64 where idx64 is set, else int32.
 * One stable radix sort by (dst, src) carrying the edge position, row pointers by binary search; weighted degrees are summed in a fixed
 * order over a second stable sort by source (integer counts without weights): no float atomics, the same bits on every run.
 * An edge with an endpoint outside [0, N) is skipped and counted in *skipped (device, accumulating; may be NULL); E = 0 is valid. */
int tgmx_cheb_laplacian(const void* src, const void* dst, int32_t idx64, const float* w, int64_t E, int64_t N, int32_t normalization,
                        float lambda_max, const float* lambda_ptr, int32_t* indptr, int32_t* cols, float* vals, float* diag,
                        void* workspace, size_t workspace_bytes, int32_t* skipped, tgmx_stream_t stream);

/* out[i, :C] = alpha (sum_{j in row i} vals[j] t[cols[j], :C] + diag[i] t[i, :C]) + beta prev[i, :C] over row-major float32 operands with
 * leading dimensions ldt / ldp / ldo (column slices of a wider operand are fine; out must not overlap t).  prev is not read when beta = 0.
 * The steps of the Chebyshev recurrence are (alpha, beta) = (1, 0) and (2, -1).  Gather form: a wave per destination row, four source
 * rows requested ahead, float4 lanes when C % 4 = 0 and every pointer / leading dimension is 16-byte aligned; a row of more than 64
 * entries is split over the four waves of its workgroup and the partial sums are added in wave order.  nnz: an upper bound on the entries
 * (the E the Laplacian was built from).  With scratch (tgmx_cheb_propagate_scratch_floats(nnz, C) floats, 16-byte aligned; 0 floats: not
 * needed) a row of more than 2048 entries leaves that launch: a second one sums it chunk by chunk of 1024 entries, a workgroup per chunk,
 * and a third adds the chunk sums in ascending order; without scratch such a row stays with its one workgroup (same values up to the order
 * of the sum, slower).  No atomics: reproducible bit for bit. */
size_t tgmx_cheb_propagate_scratch_floats(int64_t nnz, int32_t C);
int tgmx_cheb_propagate(const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N, int32_t C,
                        const float* t, int64_t ldt, const float* prev, int64_t ldp, float alpha, float beta, float* out, int64_t ldo,
                        int64_t nnz, float* scratch, size_t scratch_floats, tgmx_stream_t stream);

/* GCLSTM.forward (gclstm.py:97-107, 165-227) as ONE call, inference only: the Laplacian once (not at all for K = 1, where the cell does
 * not read the graph), op = [x | Tx_0 | ... | Tx_{K-1}] with Tx_0 = H by K - 1 propagations, pre = op W^T + b with the four gates'
 * weights stacked (rows of gate g in i, f, c, o order: [W_g^T | lins_g,0 | ... | lins_g,K-1], b = b_g + conv_g.bias), then
 * I, F, O = sigmoid, T = tanh, C_out = F C + I T, H_out = O tanh(C_out).  Every buffer is the caller's. */
typedef struct tgmx_gclstm_fwd {
  const float* x; int64_t N; int32_t in_ch, C, K, normalization;  /* [N, in_ch] */
  const void* src; const void* dst; const float* edge_w; int64_t E; int32_t idx64; float lambda_max; const float* lambda_ptr;
  const float* W; const float* b; int64_t ldw;         /* [4C, ldw >= in_ch + K C], [4C] */
  const float* H; const float* Cprev;                  /* [N, C] each */
  int32_t* indptr; int32_t* cols; float* vals; float* diag; /* [N + 1], [E], [E], [N] */
  void* lap_ws; size_t lap_ws_bytes; int32_t* skipped;
  float* prop_ws; size_t prop_ws_floats;               /* tgmx_cheb_propagate_scratch_floats(E, C) floats, or NULL */
  float* op; int64_t ldop; float* pre;                 /* [N, ldop >= in_ch + K C], [N, 4C] */
  float* H_out; float* C_out;                          /* [N, C] each */
} tgmx_gclstm_fwd_t;
int tgmx_gclstm_forward(const tgmx_gclstm_fwd_t* args, tgmx_stream_t stream);

/* ---- GCLSTM / ChebConv training (csrc/cheb_bwd.hip; composed by tgm_amd/nn/_gclstm_train.py, TGMX_GCLSTM_BWD = py | torch picks the
 * per-launch or the composed torch path instead of the one call) ---- */

/* The gate backward.  pre [N, 4C] (the forward's pre-activations, gates i, f, c, o), Cprev [N, C]; dH_out / dC_out [N, C] with leading
 * dimensions lddh / lddc, either may be NULL and then counts as zero.  I, F, T, O, C', tanh(C') are recomputed with the forward's own
 * expressions; dCn = dC' + dH' O (1 - tanh^2 C'); dpre [N, 4C] = [dCn T I(1-I) | dCn Cprev F(1-F) | dCn I (1-T^2) | dH' tanh(C') O(1-O)];
 * dCprev [N, C] = dCn F (may be NULL). */
int tgmx_gclstm_gate_backward(const float* pre, const float* Cprev, int64_t N, int32_t C, const float* dH_out, int64_t lddh,
                              const float* dC_out, int64_t lddc, float* dpre, float* dCprev, tgmx_stream_t stream);

/* tgmx_cheb_laplacian's transpose: the same L_hat as rows BY SOURCE, cols = the destinations ascending within a row, duplicates in edge
 * order.  Same arguments and workspace (tgmx_cheb_workspace_bytes); the degrees, the entry arithmetic and diag are the forward builder's
 * own code, so the multiset of (row, col, value) equals the forward's with row and col swapped, bit for bit, and diag is identical. */
int tgmx_cheb_laplacian_t(const void* src, const void* dst, int32_t idx64, const float* w, int64_t E, int64_t N, int32_t normalization,
                          float lambda_max, const float* lambda_ptr, int32_t* indptr, int32_t* cols, float* vals, float* diag,
                          void* workspace, size_t workspace_bytes, int32_t* skipped, tgmx_stream_t stream);

/* tgmx_cheb_propagate with two addends: out = alpha (M t) + beta prev + gamma prev2 (prev / prev2 are not read when their factor is 0).
 * prev or prev2 may be out itself (a lane reads the elements it writes); t must not overlap out.  Same three routes, lanes and scratch. */
int tgmx_cheb_propagate2(const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N, int32_t C,
                         const float* t, int64_t ldt, const float* prev, int64_t ldp, const float* prev2, int64_t ldp2, float alpha,
                         float beta, float gamma, float* out, int64_t ldo, int64_t nnz, float* scratch, size_t scratch_floats,
                         tgmx_stream_t stream);

/* The reverse of the Chebyshev recurrence in Clenshaw form over M = L_hat^T (tgmx_cheb_laplacian_t), K >= 2: g [N, ldg >= K C] holds the
 * gradient at Tx_k in its columns [k C, (k + 1) C) and is overwritten (b_k = g_k + 2 M b_{k+1} - b_{k+2}, k = K - 2 .. 1);
 * out [N, ldo] = g_0 + M b_1 - b_2.  K - 1 tgmx_cheb_propagate2 launches. */
int tgmx_cheb_clenshaw(const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N, int32_t C, int32_t K,
                       float* g, int64_t ldg, float* out, int64_t ldo, int64_t nnz, float* scratch, size_t scratch_floats,
                       tgmx_stream_t stream);

/* The cell's backward as ONE call (tgmx_abi_sizeof(32)).  op / ldop / pre / Cprev: what tgmx_gclstm_forward wrote and read (buffers of
 * that call).  Order: the gate backward -> d_W = x^T dpre_g (one batched tgmx_sgemm_tn, [4, in, C]) -> d_lins = dpre^T Tx_k (one batched
 * tgmx_sgemm_tn, [K, 4, C, C]: [k][g] is conv_g.lins.k.weight's) -> d_b = the column sums of dpre (one tgmx_colsum; d_conv_bias gets a
 * copy) -> d_x = dpre WT[:in]^T, the gradient at the basis = dpre WT[in:]^T (tgmx_sgemm_nt; WT [in + K C, ldwt >= 4C] is the transposed
 * stacked weight) -> K > 1: tgmx_cheb_laplacian_t (skipped edges are not counted again) and tgmx_cheb_clenshaw into d_H.  Every gradient
 * pointer may be NULL: its launches are not issued; the graph is read only for d_H with K > 1.  edge_w and lambda_max get no gradient. */
typedef struct tgmx_gclstm_bwd {
  int64_t N; int32_t in_ch, C, K, normalization;
  const float* op; int64_t ldop; const float* pre; const float* Cprev;
  const float* dH_out; int64_t lddh; const float* dC_out; int64_t lddc;   /* [N, C] each, or NULL */
  const float* WT; int64_t ldwt;
  const void* src; const void* dst; const float* edge_w; int64_t E; int32_t idx64; float lambda_max; const float* lambda_ptr;
  float* d_W; float* d_lins; float* d_b; float* d_conv_bias;              /* [4, in, C], [K, 4, C, C], [4C], [4C] */
  float* d_x; float* d_H; float* d_Cprev;                                 /* [N, in], [N, C], [N, C], contiguous */
  void* workspace; size_t workspace_bytes;                                /* tgmx_gclstm_backward_workspace_bytes(args) */
} tgmx_gclstm_bwd_t;
size_t tgmx_gclstm_backward_workspace_bytes(const tgmx_gclstm_bwd_t* args);
int tgmx_gclstm_backward(const tgmx_gclstm_bwd_t* args, tgmx_stream_t stream);

/* ---- GCNConv above the dense cap / ROLAND (the reference's tgm/nn/encoder/roland.py; GCNConv from its published PyG definition): GCN's
 * normalised adjacency as a CSR by destination, the gather SpMM over it with a fused epilogue, and ROLAND's forward as one call ---- */

/* Bytes of workspace tgmx_gcn_norm_csr needs for E edges over N nodes (0: sizes out of range). */
size_t tgmx_gcn_workspace_bytes(int64_t E, int64_t N);

/* The sparse twin of tgmx_gcn_norm_dense: D^-1/2 (A + I) D^-1/2 of the graph (src[e] -> dst[e], weight w[e] or 1) as rows BY DESTINATION:
 * indptr [N + 1], cols [E] (the sources, ascending within a row, duplicates kept in edge order), vals [E], and the diagonal diag [N].
 * gcn_norm with add_remaining_self_loops: the degree is taken over the DESTINATION index and includes the loop weight; a node's loop
 * weight is `fill` unless it has an explicit self loop, then that loop's weight (of several, the one at the highest edge position);
 * explicit loops are folded into diag; repeated edges each count; deg = 0 gives the factor 0.  add_self_loops = 0: loops are ordinary
 * entries and diag is 0.  ids int64 where idx64 is set, else int32, read as they are.
 * One stable radix sort by (dst, src) carrying the edge position, row pointers by binary search; unweighted degrees are the rows' lengths,
 * weighted ones are summed per row in CSR order by one wave: no float atomics, the same bits on every run.
 * An edge with an endpoint outside [0, N) is skipped and counted in *skipped (device, accumulating; may be NULL); E = 0 issues no sort. */
int tgmx_gcn_norm_csr(const void* src, const void* dst, int32_t idx64, const float* w, int64_t E, int64_t N, float fill,
                      int32_t add_self_loops, int32_t* indptr, int32_t* cols, float* vals, float* diag, void* workspace,
                      size_t workspace_bytes, int32_t* skipped, tgmx_stream_t stream);

#define TGMX_GCN_EPI_NONE 0  /* out = s,  s = diag[i] t[i] + sum_j vals[j] t[cols[j]] + bias */
#define TGMX_GCN_EPI_RELU 1  /* out = relu(s) */
#define TGMX_GCN_EPI_TAU 2   /* out = tau prev[i] + (1 - tau) relu(s) */

/* out[i, :C] = epi(diag[i] t[i, :C] + sum_{j in row i} vals[j] t[cols[j], :C] + bias[:C]) over row-major float32 operands with leading
 * dimensions (column slices of a wider operand are fine; out must not overlap t).  bias may be NULL.  TGMX_GCN_EPI_TAU reads prev
 * [N, ldp] and tau: from tau_ptr (device, one float: a learnable tau is never read back) when that is non-NULL, else the argument; with
 * prev_copy [N, ldc] non-NULL it also stores prev[i, :C] there (the caller's state copied on the way).  The gather, the scratch and the
 * launches are those of tgmx_cheb_propagate (scratch: tgmx_cheb_propagate_scratch_floats(nnz, C) floats); the epilogue runs wherever a
 * row finishes.  No atomics: reproducible bit for bit. */
int tgmx_gcn_propagate(const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N, int32_t C,
                       const float* t, int64_t ldt, const float* bias, int32_t epilogue, const float* prev, int64_t ldp, float tau,
                       const float* tau_ptr, float* prev_copy, int64_t ldc, float* out, int64_t ldo, int64_t nnz, float* scratch,
                       size_t scratch_floats, tgmx_stream_t stream);

#define TGMX_ROLAND_TAU 0  /* 'moving', 'learnable', None: H_l = tau prev_l + (1 - tau) relu(conv_l(.)) */
#define TGMX_ROLAND_MLP 1  /* H_l = mlp_l([relu(conv_l(.)) | prev_l]) */
#define TGMX_ROLAND_GRU 2  /* H_l = GRUCell_l(relu(conv_l(.)), prev_l) */

/* ROLAND.forward (roland.py:86-151) as ONE call (its outputs are detached in the reference, so this is the whole model whenever dropout
 * is inactive): the normalisation once, then per layer l = 0, 1 the GEMM xw = h_in W_l^T (h_in = x, then out[0]) and a propagation with
 * conv_l.bias and the update as its epilogue.  TAU: the propagation writes out[l] (prev[l] [N, ldp]; prev_copy[l] [N, C] or NULL).
 * MLP / GRU: it writes relu(.) into the left column slice of op[l] [N, 2C], whose right slice the caller has filled with prev_l;
 * MLP: out[l] = op[l] mlp_w[l]^T + mlp_b[l];  GRU: gi = op[l][:, :C] w_ih[l]^T + b_ih[l], gh = op[l][:, C:] w_hh[l]^T + b_hh[l] (two plain
 * GEMMs), then r = sigmoid(gi_r + gh_r), z = sigmoid(gi_z + gh_z), n = tanh(gi_n + r gh_n), out[l] = (1 - z) n + z prev_l.
 * Every buffer is the caller's; nothing is read back. */
typedef struct tgmx_roland_fwd {
  const float* x; int64_t N; int32_t in_ch, C, update, add_self_loops;  /* [N, in_ch] */
  const void* src; const void* dst; int64_t E; int32_t idx64; float fill;
  const float* conv_w[2]; int64_t ldw[2]; const float* conv_b[2];      /* [C, ldw[0] >= in_ch], [C, ldw[1] >= C]; [C] */
  float tau; const float* tau_ptr;                                     /* TAU */
  const float* prev[2]; int64_t ldp; float* prev_copy[2];              /* TAU */
  const float* mlp_w[2]; const float* mlp_b[2];                        /* MLP: [C, 2C], [C] */
  const float* w_ih[2]; const float* w_hh[2]; const float* b_ih[2]; const float* b_hh[2]; /* GRU: [3C, C], [3C] */
  int32_t* indptr; int32_t* cols; float* vals; float* diag;            /* [N + 1], [E], [E], [N] */
  void* norm_ws; size_t norm_ws_bytes; int32_t* skipped;
  float* prop_ws; size_t prop_ws_floats;                               /* tgmx_cheb_propagate_scratch_floats(E, C) floats, or NULL */
  float* xw;                                                           /* [N, C] */
  float* op[2];                                                        /* MLP, GRU: [N, 2C] */
  float* gi; float* gh;                                                /* GRU: [N, 3C] each */
  float* out[2];                                                       /* [N, C] each */
} tgmx_roland_fwd_t;
int tgmx_roland_forward(const tgmx_roland_fwd_t* args, tgmx_stream_t stream);

/* ---- GCNConv / TGCN over the sparse adjacency, training included (csrc/gcn_bwd.hip, csrc/tgcn.hip; composed by
 * tgm_amd/nn/_gcn_sparse_train.py, TGMX_TGCN_BWD = py | torch picks the per-launch or the composed torch path) ---- */

/* Bytes of workspace tgmx_csr_transpose needs for nnz entry slots over N nodes (0: sizes out of range). */
size_t tgmx_csr_transpose_workspace_bytes(int64_t nnz, int64_t N);

/* The transpose of a CSR in the layout of tgmx_gcn_norm_csr / tgmx_cheb_laplacian: (indptr [N + 1], cols [nnz], vals [nnz]) by row becomes
 * (indptr_t, cols_t [nnz], vals_t [nnz]) by column index; the diagonal is its own transpose (diag_t, when given and not diag itself, gets
 * a copy).  nnz: the entry SLOTS (the E the CSR was built from); only the first indptr[N] hold entries (the builders leave dropped edges
 * behind the rows) and that count is read on the device.  Every entry's row is expanded from indptr by one wave per row, then ONE stable
 * radix sort of the keys (col << cb | row) carrying the entry position, row pointers by binary search, vals_t[u] = vals[pos[u]]: values
 * are copied, not recomputed, so the multiset of (row, col, value) is the input's with row and col swapped, bit for bit; within a
 * transposed row the columns ascend and equal (row, col) entries keep the input's entry order; indptr_t[N] = indptr[N].  No float atomics;
 * nnz = 0 issues no sort.  Propagating over the result is tgmx_gcn_propagate with no bias and TGMX_GCN_EPI_NONE. */
int tgmx_csr_transpose(const int32_t* indptr, const int32_t* cols, const float* vals, const float* diag, int64_t N, int64_t nnz,
                       int32_t* indptr_t, int32_t* cols_t, float* vals_t, float* diag_t, void* workspace, size_t workspace_bytes,
                       tgmx_stream_t stream);

/* GCNConv's backward as ONE call (tgmx_abi_sizeof(39)); its forward is out = A_hat (x W^T) + b by tgmx_sgemm_nt and tgmx_gcn_propagate.
 * Order: d_b = colsum(dout) -> the transposed CSR (tgmx_csr_transpose into the workspace, unless indptr_t / cols_t / vals_t hand it in
 * built: then indptr / cols / vals are not read) -> dY = A_hat^T dout (one tgmx_gcn_propagate) -> d_W = dY^T x (tgmx_sgemm_tn, [C, in]:
 * lin.weight's layout) -> d_x = dY W (tgmx_sgemm_nt on WT [in, ldwt >= C]).  Every gradient pointer may be NULL: its launches are not
 * issued.  The adjacency gets no gradient (edge weights are data).  No float atomics: two runs give the same bits. */
typedef struct tgmx_gcn_conv_bwd {
  int64_t N; int32_t in_ch, C;
  const float* x; int64_t ldx;                      /* [N, ldx >= in_ch] (d_W) */
  const float* WT; int64_t ldwt;                    /* lin.weight transposed (d_x) */
  const float* dout; int64_t lddo;                  /* [N, lddo >= C] */
  const int32_t* indptr; const int32_t* cols; const float* vals; const float* diag; int64_t nnz; /* the forward's CSR, nnz entry slots */
  const int32_t* indptr_t; const int32_t* cols_t; const float* vals_t;                           /* its transpose already built, or NULL */
  float* d_W; float* d_b; float* d_x;               /* [C, in], [C], [N, in], contiguous */
  void* workspace; size_t workspace_bytes;          /* tgmx_gcn_conv_backward_csr_workspace_bytes(args) */
} tgmx_gcn_conv_bwd_t;
size_t tgmx_gcn_conv_backward_csr_workspace_bytes(const tgmx_gcn_conv_bwd_t* args);
int tgmx_gcn_conv_backward_csr(const tgmx_gcn_conv_bwd_t* args, tgmx_stream_t stream);

/* The TGCN cell's forward over the sparse adjacency as ONE call (tgmx_abi_sizeof(40)): tgmx_gcn_norm_csr (not with csr_built: indptr / cols
 * / vals / diag then hold the CSR already and the edge list is not read) -> xw = x W3^T as [N, 3C] (no transposed copy) -> ONE
 * tgmx_gcn_propagate over the 3C columns with b3 as its bias -> G; per gate u, r, c tgmx_tgcn_concat and its Linear, tgmx_tgcn_output: as
 * tgmx_tgcn_forward.  save != 0 is the saving form for training: gate g writes cat[g] (else all three use cat[0]); pre[0..2] are kept
 * either way; both forms give the same bits.  ids int64 where idx64 is set, else int32, read as they are; E: the edge count = the CSR's
 * entry slots.  prop_ws: tgmx_cheb_propagate_scratch_floats(E, 3 C) floats, or NULL. */
typedef struct tgmx_tgcn_csr_fwd {
  const float* x; int64_t ldx; int64_t N; int32_t in_ch, C;
  const void* src; const void* dst; const float* edge_w; int64_t E; int32_t idx64; float fill; int32_t add_self_loops, csr_built, save;
  const float* W3; int64_t ldw3; const float* b3;   /* stacked GCN weights [3 C, ldw3 >= in_ch] and biases [3 C] */
  const float* lin_w[3]; const float* lin_b[3];     /* linear_{u,r,c}: [C, 2 C], [C] */
  const float* H;                                   /* [N, C] */
  int32_t* indptr; int32_t* cols; float* vals; float* diag; /* [N + 1], [E], [E], [N] */
  void* norm_ws; size_t norm_ws_bytes; int32_t* skipped;    /* tgmx_gcn_workspace_bytes(E, N); the counter of skipped edges or NULL */
  float* prop_ws; size_t prop_ws_floats;
  float* xw; float* G;                              /* [N, 3 C] each */
  float* cat[3]; float* pre[3];                     /* [N, 2 C], [N, C] */
  float* out;                                       /* [N, C] */
} tgmx_tgcn_csr_fwd_t;
int tgmx_tgcn_forward_csr(const tgmx_tgcn_csr_fwd_t* args, tgmx_stream_t stream);

/* dG [N, 3C] = [dcat_u[:, :C] | dcat_r[:, :C] | dcat_c[:, :C]]: the left halves of the three gates' input gradients ([N, 2C] each, contiguous)
 * side by side -- the gradient at G = A_hat (x W3^T) + b3, the operand of the backward's one propagate. */
int tgmx_tgcn_gather_left(const float* dcat_u, const float* dcat_r, const float* dcat_c, int32_t C, int64_t N, float* dG, tgmx_stream_t stream);

/* The cell's backward over the sparse adjacency as ONE call (tgmx_abi_sizeof(41)): the arithmetic of the dense training path with
 * A_hat^T dG as one propagate over the transposed CSR.  x / H / cat / pre: what the saving forward read and kept; lin_wT[g] [2C, C] and
 * W3T [in, ldw3t >= 3C]: the weights transposed; dout [N, C] contiguous.  Order: tgmx_tgcn_gate_backward -> d cat_g = d pre_g W_g
 * (tgmx_sgemm_nt) with the two tgmx_tgcn_reset_backward calls in between -> d_lw[g] = d pre_g^T cat_g ([C, 2C]), d_lb[g] (tgmx_sgemm_tn,
 * tgmx_colsum) -> dG [N, 3C] = the left halves of the three d cat side by side (one gather launch) -> d_b3 = colsum(dG) -> the transposed
 * CSR (as in tgmx_gcn_conv_backward_csr: built once into the workspace unless handed in) -> dY = A_hat^T dG (ONE tgmx_gcn_propagate) ->
 * d_W3 = dY^T x ([3C, in]: the rows of gate g are conv_g.lin.weight's gradient) -> d_x = dY W3.  d_H [N, C] gets the state's gradient.
 * Every gradient pointer may be NULL.  The adjacency gets no gradient.  No float atomics: two runs give the same bits. */
typedef struct tgmx_tgcn_csr_bwd {
  int64_t N; int32_t in_ch, C;
  const float* x; int64_t ldx; const float* H;
  const float* W3T; int64_t ldw3t; const float* lin_wT[3];
  const float* cat[3]; const float* pre[3];
  const float* dout;
  const int32_t* indptr; const int32_t* cols; const float* vals; const float* diag; int64_t nnz;
  const int32_t* indptr_t; const int32_t* cols_t; const float* vals_t;
  float* d_W3; float* d_b3; float* d_lw[3]; float* d_lb[3]; float* d_x; float* d_H;
  void* workspace; size_t workspace_bytes;          /* tgmx_tgcn_backward_csr_workspace_bytes(args) */
} tgmx_tgcn_csr_bwd_t;
size_t tgmx_tgcn_backward_csr_workspace_bytes(const tgmx_tgcn_csr_bwd_t* args);
int tgmx_tgcn_backward_csr(const tgmx_tgcn_csr_bwd_t* args, tgmx_stream_t stream);

/* ---- HistoricalNegativeEdgeSamplerHook (the reference's tgm/hooks/negatives/sampler.py:68-238): per-source history on the device ---- */

/* A source's past destinations, in arrival order, as a chain of segments in `pool` (int32 words): segment k holds ranks
 * [4 (2^k - 1), 4 (2^(k+1) - 1)) in 1 + 4 2^k words, word 0 the pool offset of segment k - 1 (-1 for k = 0).  cnt [num_nodes]: past events
 * per source (zeroed when new); tail [num_nodes]: offset of the source's newest segment (whatever where cnt is 0).  state: two int32,
 * {pool_top, status}, zeroed when new: segments are handed out by atomicAdd on pool_top and never move, so offsets survive the caller
 * copying the pool into a larger one.  A stream of `count` events over num_nodes ids needs at most
 * (9 count + 11 min(count, num_nodes)) / 4 + 1 words (csrc/histneg.hip derives it); the caller sizes pool_cap from that before a call.
 * status, sticky bits: 1 = a source id outside [0, num_nodes) was offered (it draws -1 and joins no history), 2 = the pool was too small
 * for a group (its events were dropped from the chains) or a chain led outside it.  memory: the reference's [2, mem_cap] int32 log of
 * (src, dst) in arrival order, `count` events in it before this call. */
typedef struct tgmx_histneg {
  int32_t* cnt; int32_t* tail; int64_t num_nodes;
  int32_t* pool; int64_t pool_cap;
  int32_t* state;
  int32_t* memory; int64_t mem_cap; int64_t count;
  uint64_t seed, call;                                          /* the draw's generator: counter_u32(seed, call, source id) */
} tgmx_histneg_t;
size_t tgmx_histneg_workspace_bytes(int64_t B, int64_t num_nodes);

/* One batch of the hook, on `stream`: (a) one lane per position i draws neg[i] = history[umulhi32(counter_u32(seed, call, src[i]), n)] from
 * the n = cnt[src[i]] destinations stored BEFORE this batch (-1 where n = 0 or the id is out of range), valid[i] = neg[i] != -1,
 * neg_time[i] = time[i], and logs (src[i], dst[i]) at memory[:, count + i]; (b) a stable radix sort of (source, position) groups the batch,
 * one lane per group allocates and links the segments the group needs and advances cnt / tail, then every event stores its destination
 * at rank cnt_before + (its place in the group), so same-source events keep batch order.  neg / valid NULL together: no draw (the first
 * batch); time / neg_time NULL together: no copy.  ids int64 where the *_is64 flag is set, else int32.  Four launches while the sort is
 * one (B within rocPRIM's single-block limit); nothing is read back. */
int tgmx_histneg_step(const tgmx_histneg_t* h, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const int64_t* time,
                      int64_t B, int32_t* neg, int64_t* neg_time, uint8_t* valid, void* workspace, size_t workspace_bytes,
                      tgmx_stream_t stream);

/* ---- the decoders (the reference's tgm/nn/decoder/{link,node,graph}proppred.py, tgm/nn/modules/aggregation.py): an MLP head over merged
 * pairs of embedding rows, over rows, or over one pooled row.  Every entry sums in one fixed order: a call is reproducible bit for bit. ---- */

#define TGMX_DECODER_ACT_NONE 0
#define TGMX_DECODER_ACT_RELU 1

/* C[R, N] = act(A1[ia] Wa^T + A2[ib] Wb^T + bias): row r of the first operand is A1[ia[r], :K1] (ia NULL: row r), likewise the second;
 * A2 = NULL is the one-operand case.  Wa [N, ldwa >= K1], Wb [N, ldwb >= K2], bias [N] or NULL.  Exact-fp32 MFMA (16x16x4), the rows
 * gathered into LDS through the indices; the K loop runs through the first operand and then the second in 64-wide chunks, ascending (inside a
 * chunk four interleaved sets of 4-wide k-steps, folded pairwise).  n1 / n2: rows of A1 /
 * A2.  An index outside [0, n) is not dereferenced: row r of C is NaN and *bad (device, accumulating; may be NULL) counts it. */
int tgmx_decoder_pair_gemm(const float* A1, int64_t lda1, int64_t n1, const int32_t* ia, const float* A2, int64_t lda2, int64_t n2,
                           const int32_t* ib, const float* Wa, int64_t ldwa, int32_t K1, const float* Wb, int64_t ldwb, int32_t K2,
                           const float* bias, int32_t act, float* C, int64_t ldc, int64_t R, int32_t N, int32_t* bad, tgmx_stream_t stream);

/* The table form's per-pair stage over P [NP, ldp >= 2H] (P = z [Wa ; Wb]^T + [bias | 0]): h = act(P[a, :H] + P[c, H:2H]) for
 *   M >= 0: B queries; query b pairs a = ia[b] with c = ib[b] (candidate 0) and with its candidates neg[b M + j - 1] (off NULL: M each) or
 *           neg[off[b] + j - 1] (off [B + 1], int64; max_candidates: the longest list, a host number); pair j of query b is output row
 *           b (M + 1) + j, or off[b] + b + j.  A workgroup loads the query's half row once and reuses it for its candidates;
 *   M = -1: B flat pairs, a = ia[r], c = ib[r], output row r.
 * out_dim in 1..16: out[row, :out_dim] = h w_last^T + b_last (w_last [out_dim, H]);  out_dim = 0: out[row, :H] = h (leading dimension ldo).
 * Lanes span H and fold by a fixed butterfly; for H < 64 several pairs share a wave.  ids int64 where idx64 is set, else int32.  An index
 * outside [0, NP) is not dereferenced: the pair's outputs are NaN and *bad counts it.  TGMX_E_UNSUPPORTED for H > 512 or out_dim > 16. */
int tgmx_decoder_score(const float* P, int64_t ldp, int64_t NP, int32_t H, const void* ia, const void* ib, const void* neg, int32_t idx64,
                       const int64_t* off, int64_t M, int64_t max_candidates, int64_t B, int32_t act, const float* w_last, const float* b_last,
                       int32_t out_dim, float* out, int64_t ldo, int32_t* bad, tgmx_stream_t stream);

/* out[r, :out_dim] = x[r, :K] W^T + b as row dots, out_dim <= 16 (W [out_dim, K] contiguous); TGMX_E_UNSUPPORTED beyond that (a wider last
 * layer is a tgmx_sgemm_nt). */
int tgmx_decoder_tail(const float* x, int64_t ldx, int64_t R, int32_t K, const float* W, const float* b, int32_t out_dim, float* out,
                      tgmx_stream_t stream);

/* out[:D] = the column sum (mean != 0: the column mean, sum / N) of x [N, D].  Chunks of 128 rows, then the chunks, each level
 * in four interleaved chains folded pairwise, in double, rounded to float32 once: the order depends on N alone, no atomics.  scratch: tgmx_pool_rows_scratch_floats(N, D) floats, 8-byte aligned (0 for N <= 128).
 * TGMX_E_UNSUPPORTED for D > 1536. */
size_t tgmx_pool_rows_scratch_floats(int64_t N, int32_t D);
int tgmx_pool_rows(const float* x, int64_t ldx, int64_t N, int32_t D, int32_t mean, float* scratch, size_t scratch_floats, float* out,
                   tgmx_stream_t stream);

#define TGMX_DECODER_MAX_LAYERS 8
#define TGMX_DECODER_ROWS 0   /* the layers over a1 [R, D] (NodePredictor), or over its pooled row (GraphPredictor) */
#define TGMX_DECODER_PAIR 1   /* merge = tgmx_decoder_pair_gemm into h[1] [R, H], then the layers */
#define TGMX_DECODER_TABLE 2  /* merge = P = a1 wa^T + mbias (wa [2H, ldwa] stacked, mbias [2H]) and tgmx_decoder_score, then the layers */
#define TGMX_DECODER_POOL_NONE 0
#define TGMX_DECODER_POOL_MEAN 1
#define TGMX_DECODER_POOL_SUM 2

typedef struct tgmx_decoder_layer {
  const float* w; const float* b; int32_t in, out;    /* Linear: [out, in], [out] */
} tgmx_decoder_layer_t;

/* One row x [layers[0].in] through num_layers Linears (relu between, none after the last) into out [layers[last].out]: one workgroup, the
 * row in LDS, each dot accumulated in double and rounded once.  TGMX_E_UNSUPPORTED for a layer wider than 4096. */
int tgmx_decoder_row_mlp(const float* x, const tgmx_decoder_layer_t* layers, int32_t num_layers, float* out, tgmx_stream_t stream);

/* A whole head as ONE call.  layers: the Linears after the merge stage, relu between them and none after the last (ConcatMerge: the first
 * Linear of the model IS the merge stage, with merge_act = relu; LearnableSumMerge: the merge stage is lin_src / lin_dst with merge_act =
 * none and every Linear of the model is a layer).  A last layer of at most 16 outputs is tgmx_decoder_tail -- in the table form with one
 * layer it rides tgmx_decoder_score -- the others are tgmx_sgemm_nt flipping between h[0] and h[1] ([R, widest hidden layer] each); for R = 1 the
 * layers are one tgmx_decoder_row_mlp.
 * PAIR: ia / ib are int32 (or NULL).  TABLE: ia, ib, neg, off, M, max_candidates, B as in tgmx_decoder_score; R: output rows in all.
 * Every buffer is the caller's; nothing is read back. */
typedef struct tgmx_decoder_fwd {
  int32_t form, merge_act, pool, num_layers;
  const float* a1; int64_t lda1, n1; const float* a2; int64_t lda2, n2;
  const void* ia; const void* ib; const void* neg; const int64_t* off; int32_t idx64, reserved_; int64_t M, max_candidates, B, R;
  const float* wa; int64_t ldwa; const float* wb; int64_t ldwb; const float* mbias; int32_t D, H;
  tgmx_decoder_layer_t layers[TGMX_DECODER_MAX_LAYERS];
  float* P; float* h[2]; float* pooled; float* pool_ws; size_t pool_ws_floats; int32_t* bad; float* out;
} tgmx_decoder_fwd_t;
int tgmx_decoder_forward(const tgmx_decoder_fwd_t* args, tgmx_stream_t stream);

/* ---- decoder training (csrc/decoder_bwd.hip): the saving forward and the backward of the ROWS, PAIR and flat TABLE heads, ONE call each.
 * No float atomics anywhere: every sum has one fixed order, two runs give the same bits. ---- */

/* The last layer's backward, out_dim <= 16 (the tgmx_decoder_tail case): dout [R, out_dim], x [R, K] the layer's saved input, W [out_dim, K]:
 *   dx[r, j] = (relu == 0 || x[r, j] > 0) * sum_o dout[r, o] W[o, j]   (ascending o; the mask reads the saved activation, x == 0 gives 0)
 *   dW[o, j] = sum_r dout[r, o] x[r, j],  db[o] = sum_r dout[r, o]
 * A workgroup owns a block of rows (their number follows R: 4 up to R = 1024, at most 256 blocks) and 64 columns; its four waves take the
 * block's rows in turn, their partial sums add in wave order, and a second launch adds the blocks' partials in ascending block order.
 * dx, dW, db may each be NULL (not computed).  workspace: tgmx_decoder_tail_bwd_workspace_floats() floats (0 when dW and db are NULL).
 * R = 0 writes nothing.  TGMX_E_UNSUPPORTED for out_dim > 16. */
size_t tgmx_decoder_tail_bwd_workspace_floats(int64_t R, int32_t K, int32_t out_dim);
int tgmx_decoder_tail_bwd(const float* dout, int64_t lddout, const float* x, int64_t ldx, int64_t R, int32_t K, const float* W, int32_t out_dim,
                          int32_t relu, float* dx, int64_t lddx, float* dW, float* db, float* workspace, size_t workspace_floats,
                          tgmx_stream_t stream);

/* The table form's scatter: dP [NP, 2H] (contiguous) from dh [R, H] and the pairs (ia[r], ib[r]):
 *   dP[n, :H] = sum_{r: ia[r] = n} dh[r],  dP[n, H:] = sum_{r: ib[r] = n} dh[r]
 * read back through an inverted index: keys ((n or NP + n) << cb | r), one rocPRIM radix sort, row pointers by binary search (edge_csr.h),
 * then spmm.h's gather (a row's pairs add in ascending r; rows of more than 64 / 2048 pairs take its fixed-order splits).  Every row of dP
 * is written, rows without a pair as zeros.  A pair with an index outside [0, NP) is dropped from both halves and never dereferenced.
 * ids int64 where idx64 is set, else int32.  2R < 2^31, 2NP < 2^31. */
size_t tgmx_decoder_scatter_workspace_bytes(int64_t R, int64_t NP, int32_t H);
int tgmx_decoder_scatter(const float* dh, int64_t lddh, int64_t R, int32_t H, const void* ia, const void* ib, int32_t idx64, int64_t NP,
                         float* dP, void* workspace, size_t workspace_bytes, tgmx_stream_t stream);

/* For every job: dst[r, :C] = src[r, :C] (src NULL: dst as it is) where both of pair r's indices lie in [0, NP), zeros elsewhere.  ONE
 * launch: the backward's first in the table form, over the upstream gradient and every saved activation (a dropped pair's rows are NaN). */
typedef struct tgmx_drop_job {
  const float* src; float* dst; int64_t lds, ldd; int32_t C, reserved_;
} tgmx_drop_job_t;
int tgmx_decoder_drop_rows(const void* ia, const void* ib, int32_t idx64, int64_t NP, int64_t R, const tgmx_drop_job_t* jobs, int32_t n_jobs,
                           tgmx_stream_t stream); /* n_jobs <= TGMX_DECODER_MAX_LAYERS + 1 */

/* The training argument block (tgmx_abi_sizeof(30)).  fwd: the head as tgmx_decoder_forward takes it, with these differences: pool is
 * NONE; TABLE takes flat pairs only (M = -1) and reads the merge weights WHERE THE PARAMETERS ARE, as PAIR does (wa, wb [H, ld >= D],
 * two GEMMs into the halves of P; nothing stacked per step); fwd.h is not used.  The forward keeps what the backward reads in buffers of
 * THIS call: act[0] [R, H] the merge stage's output (PAIR, TABLE; the table form never fuses the last layer into tgmx_decoder_score),
 * act[l] [R, layers[l].in] the input of layer l >= 1.  ROWS reads a1 as layer 0's input (act[0] unused).
 * Backward: dout [R, out_dim] with leading dimension lddout.  Every gradient pointer may be NULL: that gradient's launch is not issued.
 * d_a1 [R, D] (TABLE: [n1, D]) and d_a2 [R, D] contiguous; d_wa / d_wb [H, D] with their leading dimensions (ConcatMerge: the column halves
 * of the first Linear's gradient, ld 2D); d_mbias, d_mbias2 [H] both receive the merge bias's gradient; d_w[l] / d_b[l] as layers[l].
 * Order: [TABLE: tgmx_decoder_drop_rows] -> the weights transposed (one tgmx_pack2d) -> the last layer (tgmx_decoder_tail_bwd, or the
 * generic route) -> the hidden layers from the back (dW: tgmx_sgemm_tn, db: tgmx_colsum, dX: tgmx_sgemm_nt on the transposed weight,
 * tgmx_relu_mask) -> the merge stage (PAIR: two tgmx_sgemm_tn, tgmx_colsum, two tgmx_sgemm_nt; TABLE: tgmx_decoder_scatter, then the same
 * over the NP rows of dP, one tgmx_sgemm_nt with K = 2H for d_a1).  In the table form the saved activations of a dropped pair are zeroed
 * in place.  workspace: tgmx_decoder_backward_workspace_bytes(). */
typedef struct tgmx_decoder_train {
  tgmx_decoder_fwd_t fwd;
  float* act[TGMX_DECODER_MAX_LAYERS];
  const float* dout; int64_t lddout;
  float* d_a1; float* d_a2; float* d_wa; int64_t ld_dwa; float* d_wb; int64_t ld_dwb; float* d_mbias; float* d_mbias2;
  float* d_w[TGMX_DECODER_MAX_LAYERS]; float* d_b[TGMX_DECODER_MAX_LAYERS];
  void* workspace; size_t workspace_bytes;
} tgmx_decoder_train_t;
int tgmx_decoder_forward_save(const tgmx_decoder_train_t* args, tgmx_stream_t stream);
size_t tgmx_decoder_backward_workspace_bytes(const tgmx_decoder_train_t* args);
int tgmx_decoder_backward(const tgmx_decoder_train_t* args, tgmx_stream_t stream);

/* ---- BatchAnalyticsHook, EdgeEventsSeenNodesTrackHook, NodeAnalyticsHook (the reference's tgm/hooks/analytics/, tgm/hooks/node_tracks.py):
 * distinct counts within a batch, membership in sets that grow over the stream, an ordered compaction (csrc/analytics.hip) ---- */

#define TGMX_AN_BAD_ID 1     /* status bits: an id outside [0, num_nodes) was offered (the event took no part) */
#define TGMX_AN_TABLE_FULL 2 /*              a claim found no room in a pair table (the host's capacity rule makes that a bug) */
#define TGMX_AN_BAD_TIME 4   /*              a negative time was offered (the pair tables' empty key is all ones; the event took no part) */

/* One batch as the analytics hooks read it.  Any pointer may be NULL (the field is None) with its count 0; src and dst go together.  E edges,
 * Et edge times (E, or 0 without edge_time), Nn node events, Nt node times (Nn, or 0 without node_x_time).  Integer vectors are int64 where
 * their *_is64 flag is set, else int32. */
typedef struct tgmx_an_batch {
  const void* src; const void* dst; int64_t E; int32_t src_is64, dst_is64;
  const void* edge_time; int64_t Et; int32_t edge_time_is64, reserved0_;
  const void* nids; int64_t Nn; int32_t nids_is64, reserved1_;
  const void* node_time; int64_t Nt; int32_t node_time_is64, reserved2_;
} tgmx_an_batch_t;

/* out [8] int64 (device): 0 E, 1 Nn, 2 distinct values of edge_time u node_time (time_as_f32 != 0: of the values rounded to float32, the
 * reference's count when exactly one of the two fields is None), 3 distinct ids of src u dst u nids, 4 the float32 quotient
 * (float)(2 E) / (float)out[7] in the word's first four bytes (0.0f without edges), 5 E - distinct (src, dst, time) triples (0 unless
 * Et = E), 6 Nn - distinct (nid, time) pairs (0 unless Nt = Nn), 7 distinct ids of src u dst.  Five batch-local hash sets in `workspace`,
 * each a power of two >= 2 x its keys of int32 slots holding the index of the key that claimed them; three launches (reset, insert,
 * finish), nothing read back.  Sizes below 2^28.  Every count is an integer sum: the result does not depend on scheduling. */
size_t tgmx_batch_analytics_workspace_bytes(int64_t E, int64_t Et, int64_t Nn, int64_t Nt);
int tgmx_batch_analytics(const tgmx_an_batch_t* batch, int32_t time_as_f32, int64_t* out, void* workspace, size_t workspace_bytes,
                         tgmx_stream_t stream);

/* mask [num_nodes] bytes.  First launch: mask[id] = 1 for every id of src and dst (ids outside [0, num_nodes) set TGMX_AN_BAD_ID in
 * state[1] and store nothing).  Second launch (Ny > 0), one workgroup: the positions i of nids [Ny] with mask[nids[i]] != 0, ascending, into
 * out_pos, the ids there into out_ids (an array of nids' type), their number into state[0].  state: two int64 {count, status}, status
 * accumulating; the caller reads both at once. */
int tgmx_seen_nodes_step(uint8_t* mask, int64_t num_nodes, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, int64_t E,
                         const void* nids, int32_t nids_is64, int64_t Ny, int64_t* out_pos, void* out_ids, int64_t* state,
                         tgmx_stream_t stream);

/* NodeAnalyticsHook's state.  slot_of [num_nodes]: index of a tracked node in [0, T), or -1.  first_seen / last_seen [T]: -1 = never.
 * appearances [T].  Four pair tables (slots as tgmx_edgebank_t's, empty key all ones, capacities powers of two): edges key = src << 32 | dst;
 * nbrs key = tracked index << 32 | neighbour; times key = the timestamp, value = its dense id in [0, 2^32); apps key = tracked index << 32
 * | time id.  counters [8] int64: 0 distinct times so far (the next dense id), 1-3 occupancy of edges / nbrs / apps, 4 status
 * (TGMX_AN_* bits, accumulating), 5 entries moved by rehashes.  Per-call scratch, zeroed when new and left zero by every call: degree / new_nbrs / present [T] int32,
 * scalars [16] int64.  stamp [num_nodes] int32, zeroed when new: the number of the last call that met the node as an edge endpoint. */
typedef struct tgmx_node_analytics {
  const int32_t* slot_of; int64_t num_nodes, T;
  int64_t* first_seen; int64_t* last_seen; int64_t* appearances;
  void* edges; int64_t edges_cap; void* nbrs; int64_t nbrs_cap; void* times; int64_t times_cap; void* apps; int64_t apps_cap;
  int64_t* counters;
  int32_t* degree; int32_t* new_nbrs; int32_t* present; int32_t* stamp; int64_t* scalars;
} tgmx_node_analytics_t;

/* One batch, `call` = 1, 2, ... over the state's life.  Events with an id outside [0, num_nodes) or a negative time take no part (status
 * bits).  Time pass: every time claims its slot in `times` (a new one takes the next dense id) and folds into the batch maximum.  Event pass:
 * every edge claims (src, dst) in `edges`; per tracked endpoint degree + 1, (endpoint, other end) claimed in `nbrs`, (endpoint, time)
 * in `apps`; per node event (node, time) in `apps`.  Finalise writes out [T + 2, 8] int64:
 *   row i < T: {2, degree, appearances, new neighbours, current - first_seen, 0, 0, 0} for a tracked node present in the batch (first_seen
 *              set if it was -1, last_seen = current), {1, 0, appearances, 0, last - first, current - last, 0, 0} for one seen before, zeros else;
 *   row T:     {distinct times so far, pairs new to `edges`, distinct edge endpoints of this batch, edges taking part, node events taking part,
 *              node events of untracked ids, current = max(times of the batch, 0), status};
 *   row T + 1: {occupancy of edges, nbrs, times, apps, 0, 0, 0, 0}.
 * Three launches, integer atomics only, nothing read back. */
int tgmx_node_analytics_step(const tgmx_node_analytics_t* st, const tgmx_an_batch_t* batch, int64_t call, int64_t* out, tgmx_stream_t stream);

/* Every entry of the pair table `from` moves into `to` (to_cap slots, all empty).  state: two int64, counters + 4 of the state above:
 * {status: TGMX_AN_TABLE_FULL where a claim found no room; entries moved, accumulating}. */
int tgmx_node_analytics_rehash(const void* from, int64_t from_cap, void* to, int64_t to_cap, int64_t* state, tgmx_stream_t stream);

/* ---- TGBNegativeEdgeSamplerHook and its thgl / tkgl kin (the reference's tgm/hooks/negatives/tgb_sampler.py): the evaluation set of a
 * split, constant for its life, as a table on the device; a batch of positives is answered without a loop on the host. ----
 *
 * The set, flattened by the host: keys [P, 4] int64 (unused fields 0), row p's negatives at pool[indptr[p] .. indptr[p] + rowlen[p]) with
 * indptr [P + 1] a multiple of four everywhere (a row is read with 16-byte loads) and the gaps filled with -1.  slots [capacity] int32, a
 * power of two > P, all -1 when new: open addressing, linear probing, a slot holds a row index; after tgmx_tgbneg_build it is read-only.
 * field[j]: which batch vector key column j is compared with (0 src, 1 dst, 2 time, 3 edge type, -1: the column is 0).  bitmap
 * [bitmap_words] uint32 over the ids [0, 32 bitmap_words), zeroed when new and left zero by every call (more than
 * tgmx_tgbneg_limit(1) words: a multiple of tgmx_tgbneg_limit(2)); first_missing: one int32, 2^31 - 1 when new and after every call;
 * block_counts [num_blocks >= bitmap_words / tgmx_tgbneg_limit(2), rounded up] int32 scratch.  qpad: the longest row rounded up to four. */
#define TGMX_TGBNEG_DUPLICATE 1
#define TGMX_TGBNEG_FULL 2
typedef struct tgmx_tgbneg {
  const int64_t* keys; const int64_t* indptr; const int32_t* rowlen; const int32_t* pool;
  int64_t P, pool_ints;
  int32_t* slots; int64_t capacity;
  uint32_t* bitmap; int64_t bitmap_words;
  int32_t* first_missing; int32_t* block_counts; int64_t num_blocks;
  int32_t qpad; int32_t field[4]; int32_t reserved;
} tgmx_tgbneg_t;

/* which: 0 = the largest qpad a single wave copies (longer rows take a workgroup per positive), 1 = the largest bitmap_words the
 * one-workgroup compaction takes (larger bitmaps take count / scan / write), 2 = bitmap words per workgroup of that split. */
int64_t tgmx_tgbneg_limit(int32_t which);

/* Inserts the P rows (one lane each; a slot is claimed by a 32-bit compare-and-swap, a taken slot's key is read from `keys`).  status: one
 * int32, accumulating TGMX_TGBNEG_DUPLICATE (two rows with one key) and TGMX_TGBNEG_FULL (no free slot in `capacity` probes). */
int tgmx_tgbneg_build(const tgmx_tgbneg_t* t, int32_t* status, tgmx_stream_t stream);

/* One batch of B > 0 positives; src / dst / time / etype are int64 where their *_is64 flag is set, else int32 (etype may be NULL when no
 * key column names it).  Launch 1, one wave (qpad <= limit 0) or one workgroup per positive: a wave-uniform probe, then row b of matrix
 * [B, qpad] int32 = the key's negatives, -1 behind them, every id marked in the bitmap (an atomicOr only where a plain load shows the bit
 * clear); a key that is not in the table leaves a row of -1 and folds b into first_missing by atomicMin.  Then the ordered compaction of
 * the bitmap into neg (ascending ids, at most neg_cap of them written), which clears every word it read: one workgroup, or count / scan /
 * write.  Its tail writes stats: int64 {ids written to neg, min(time), max(time), lowest missing b or -1}, then the B row lengths as int32
 * from byte 32 on.  Integer atomics only; the result does not depend on scheduling; nothing is read back. */
int tgmx_tgbneg_query(const tgmx_tgbneg_t* t, const void* src, int32_t src_is64, const void* dst, int32_t dst_is64, const void* time,
                      int32_t time_is64, const void* etype, int32_t etype_is64, int64_t B, int32_t* matrix, int32_t* neg, int64_t neg_cap,
                      int64_t* stats, tgmx_stream_t stream);

/* The same compaction and tail for a matrix [B, qpad] the caller filled (-1 = no id): only bitmap, bitmap_words, first_missing, block_counts,
 * num_blocks and qpad of `t` are read.  The row lengths in stats are left as they are. */
int tgmx_tgbneg_unique(const tgmx_tgbneg_t* t, const int32_t* matrix, int64_t B, const void* time, int32_t time_is64, int32_t* neg,
                       int64_t neg_cap, int64_t* stats, tgmx_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TGM_AMD_H */
