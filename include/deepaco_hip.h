/*
 * deepaco_hip.h -- C ABI of libdeepaco_hip.so: DeepACO's ant-rollout hot path on MI355X (gfx950).
 *
 * This is the drop-in boundary.  The reference (henry-yeh/DeepACO) has no native boundary for
 * this path: its ACO classes issue stock PyTorch ops.  Each entry point below replaces the
 * body of one reference method and is bound from Python with ctypes and tensor.data_ptr(),
 * the same mechanism the reference already uses for its one native dependency
 * (cvrp_nls/swapstar.py:134-185 loads libhgscvrp.so with ctypes).  INTEGRATION.md shows the
 * binding a maintainer would add on the reference side.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless stated; arrays are dense, row-major;
 *  - B = instances in the batch (the reference always runs B = 1), n = nodes, A = ants;
 *  - `stream` is a hipStream_t (void* here so the header needs no HIP include); all work is
 *    enqueued on it and no entry point synchronises with the host;
 *  - return value: 0 = ok, < 0 = error (see DACO_E_*); the message is in daco_last_error()
 *    (thread-local).  No entry point ever falls back to a CPU path.
 *  - the library keeps no global mutable state: entry points are re-entrant across streams
 *    and devices; scratch memory is the caller's (size from the *_workspace_bytes queries).
 */
#ifndef DEEPACO_HIP_H
#define DEEPACO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DACO_VERSION 130 /* 0.1.23: bumped whenever an entry point's signature or the draw stream of a mode changes (120: the head-row sampler; 121: head_slots; 122: scan_sparse draws once after a rejection; 123: its workspace takes the ant count; 124: daco_hgs_*, daco_cvrp_sample takes ant_gid_bstride; 125: daco_tsp_sample_heads / daco_pheromone_update_heads (the sparse workspace still begins with the dense rows P: see daco_tsp_sample_heads); 126: daco_tsp_sparse_tours_offset / the record from tours16 rows, the sparse workspace holds the u16 tours at every n); 127: daco_mkpv_*, daco_transformer_*; 128: daco_transformer_forward sums attention tile by tile, other last bits above 128 tokens; 129: daco_transformer_forward_train / daco_transformer_backward; daco_rcpsp_* were added under 129 as well: new entry points only, no signature or draw stream of an existing one changed, and a library without them fails at symbol lookup when it is loaded; daco_tsp_sparse_resident_per_cu and daco_tsp_sparse_split_tours were added under 129 in the same way, with the split-tour variant of the construction kernel: same draws, same signatures -- profiles/counters.json and profiles/hbm_traffic.json were collected again with that kernel; daco_rcpsp_net_* were added under 129 too, new entry points only, and so were daco_rcpsp_net_train_*; daco_sibling_objective / daco_sibling_record with DACO_SIB_SMTWTP / DACO_SIB_BPP were added under 129 in the same way: tests/test_mkp_grad_spec.py holds the number at 129; daco_hgs_local_search_ss / daco_hgs_workspace_bytes_ss (SWAP*) were added under 129 likewise, and so were daco_sparsify / daco_sparse_head / daco_head_stats, and daco_cvrp_knn_graph; daco_head_eta and the uniform-tail mode of the head-row path were added under 129 in the same way: same draws, same head rows, no existing signature changed; 130: one entry point per head-row call -- daco_tsp_sample_heads, daco_pheromone_update, daco_pheromone_update_heads and daco_track_best take their modes (race, uniform tail, the record kept by the update, tours16 rows) as arguments and the exports that stood beside them are gone; same draws, same kernels; daco_sop_graph_count / daco_sop_graph_fill and daco_gnn_train_forward_ragged / daco_gnn_train_backward_ragged were added under 130: new entry points only, no existing signature, result or launch sequence changed) */

/* error codes */
#define DACO_OK 0
#define DACO_E_BADARG (-1)   /* null pointer, size out of range */
#define DACO_E_TOOLARGE (-2) /* n exceeds what the kernel's register/LDS plan supports */
#define DACO_E_HIP (-3)      /* a HIP runtime call failed */
#define DACO_E_WORKSPACE (-4)/* workspace too small */

/* sampler modes */
#define DACO_RACE_NOISE 0  /* exponential race, noise read from memory (bit-exact parity mode) */
#define DACO_RACE_PHILOX 1 /* exponential race, Philox4x32-10 noise generated in-kernel */
#define DACO_SCAN 2        /* roulette / inverse-CDF by wavefront prefix scan, one uniform per step.
                            * daco_tsp_sample and daco_cvrp_sample pack four ants per wavefront for
                            * n <= 256 and two for 256 < n <= 512 (the 16- and 32-lane variants of the
                            * scan); everything else uses one ant per wavefront. */
#define DACO_SCAN_WAVE 3   /* DACO_SCAN with the one-ant-per-wavefront layout for every n: the draw
                            * daco_pick_move / daco_sibling_sample make (there it is a synonym of
                            * DACO_SCAN) */

/* limits */
#define DACO_MAX_NODES 4096

int daco_version(void);
const char *daco_last_error(void);

/* Layout helpers (the padded leading dimension the sampler uses internally; exported so the
 * oracle-side tests can state the summation order). */
int daco_vec_for_n(int n);
int daco_ld_for_n(int n);

/* ---------------------------------------------------------------------------------------------
 * daco_tsp_sample -- replaces ACO.gen_path + ACO.pick_move
 *   tsp/aco.py:134-177 (random start, Categorical normalises once -> norm_passes = 1)
 *   tsp_nls/aco.py:184-220 (start 0, explicit renormalisation  -> norm_passes = 2)
 *
 * For every instance b and ant a builds a tour of n nodes: start node, then n-1 draws from
 * p_k = tau[prev][k]^alpha * eta[prev][k]^beta * [k unvisited].
 *
 *   tau, eta   [B][n][n] f32.  tau_bstride / eta_bstride: element stride between instances
 *              (n*n for dense batches, 0 to share one matrix across the batch).
 *   mode       DACO_RACE_NOISE: action = argmax_k ((p_k/S)/q_k) with q = noise, exactly the
 *              arithmetic of torch.multinomial's one-sample path (first maximum wins);
 *              norm_passes in {0,1,2} = how many times p is divided by its row sum first.
 *              DACO_RACE_PHILOX: the same race with q_k = -log2(1-u_k), u from Philox.
 *              DACO_SCAN: r = u*S, first candidate (lane-major order) whose running sum >= r.
 *   start      [B][A] int64 or NULL.  If NULL: fixed_start >= 0 -> every ant starts there,
 *              fixed_start < 0 -> start = floor(n * u32 / 2^32) from the Philox stream.
 *   noise      DACO_RACE_NOISE: [B][n-1][A][n] f32 (the reference's q tensors, step-major), required.
 *              DACO_SCAN / DACO_SCAN_WAVE: NULL, or [B][n-1][A] f32 uniforms in (0,1) that replace the Philox
 *              stream (the reference's roulette with an injected uniform stream, tsp_nls/aco.py:266-274).
 *   seed, iter, ant_gid0   Philox key and counter words: ant (b,a) uses global ant id
 *              ant_gid0 + b*A + a; `iter` must differ between calls that should be independent.
 *   ant_gid_bstride  0, or the ant-id stride between instances when this call builds only a slice of a
 *              colony's ants: ant (b,a) then uses id ant_gid0 + b*ant_gid_bstride + a.  A rank that owns ants
 *              [lo, hi) of colonies with A_total ants passes ant_gid0 = lo, ant_gid_bstride = A_total and draws
 *              exactly the tours a single call with all A_total ants would draw for those ants.
 *   iter_offset  optional device pointer to a uint64 that the kernel adds to `iter` when it starts:
 *              a caller that captures its iteration into a HIP graph keeps the counter in device
 *              memory and bumps it inside the graph (arguments are frozen at capture).  NULL = 0.
 *   paths      out [B][n][A] int64  (reference layout: paths[:, i] is ant i's tour)
 *   logp       out [B][n-1][A] f32 or NULL: log(clamp(p_chosen/S, eps, 1-eps)), eps = 2^-23
 *   rowsum     out [B][n-1][A] f32 or NULL: S at each step (saved for daco_tsp_sample_backward)
 *   flags      out [B] int32 or NULL: set to 1 if some draw had no feasible candidate
 *              (the reference's Categorical raises ValueError there); caller zeroes it.
 *   dist, costs   optional fusion of ACO.gen_path_costs: if costs != NULL, dist [B][n][n]
 *              (dist_bstride as for tau) is read once per step and costs [B][A] receives the
 *              closed-tour length in daco_tour_costs' summation order.
 *   nbr        optional out [B][n][A] uint32: prev(node) | next(node) << 16 per (node, ant), the
 *              form daco_pheromone_update consumes (saves its own pass over `paths`).
 *   workspace  daco_tsp_sample_workspace_bytes(B, n, mode) bytes of device scratch.
 *   ev_begin, ev_end   optional hipEvent_t pair (NULL to skip) recorded on `stream` immediately
 *              before and after the tour-construction kernel itself (not the P = tau^a*eta^b
 *              pre-pass), so a caller can time the dominant kernel without a profiler.
 */
size_t daco_tsp_sample_workspace_bytes(int B, int n, int mode);
int daco_tsp_sample(void *stream, int B, int n, int A,
                    const float *tau, long tau_bstride, const float *eta, long eta_bstride,
                    float alpha, float beta, int mode, int norm_passes,
                    const int64_t *start, int fixed_start, const float *noise,
                    uint64_t seed, uint64_t iter, const uint64_t *iter_offset, uint32_t ant_gid0,
                    int ant_gid_bstride,
                    int64_t *paths, float *logp, float *rowsum, int32_t *flags,
                    const float *dist, long dist_bstride, float *costs, uint32_t *nbr,
                    void *workspace, size_t workspace_bytes, void *ev_begin, void *ev_end);

/* ---------------------------------------------------------------------------------------------
 * daco_tsp_sample_heads -- ACO.gen_path on HEAD / TAIL rows (sampler "scan_sparse"); replaces
 *   tsp/aco.py:134-177 with the roulette of tsp_nls/aco.py:260-275, for heuristics made k-sparse by
 *   tsp/aco.py:52-67 (sparsify: k live entries per row, 1e-10 elsewhere) -- the reference's inference setting.
 * The one entry point of the head-row sampler; its modes (race on head rows, head rows left by the update, uniform tail) are
 * arguments, described after the draw.
 *
 * race = 0, the scan draw.  Same distribution as daco_tsp_sample(DACO_SCAN): p_k = tau^alpha * eta^beta * [k unvisited].  A row is split into a
 * head (up to 63 or 127 candidates, head_id) and the tail (the rest).  A step draws r = u * (H + T) with H the head's
 * live mass and T the tail's static mass: inside the head -> inverse CDF over 64 / 128 slots (384 / 768 bytes instead of a
 * row of 4n); past the head -> inverse CDF over all tail entries, and if that lands on a visited one the step draws once
 * more, the dense masked draw over all open candidates with a second uniform (rejection over a superset with an exact
 * fallback: the outcome is the categorical above, a step reads the row at most twice); no live head candidate -> the
 * dense masked draw of the 64-lane scan specification.  Its own uniform stream: tours differ from DACO_SCAN's under the
 * same seed, the distribution does not.  Specification: oracle/daco_oracle.c draw_scan_sparse.
 * race = 1, the race on head rows.  daco_tsp_sample(DACO_RACE_PHILOX) on the same head rows, with the SAME tours (same seed,
 * same noise indexing by node id): the exponential race of torch.multinomial's one-sample path (tsp/aco.py:174-175) is won
 * by a head candidate whenever its key L/p is below what any tail candidate could draw, L_min / max_tail(p); that is checked
 * every step and the dense race runs for the ant otherwise.  head_slots variates per step instead of n.
 *   129 <= n <= 1024.
 *   head_slots  64 or 128: slots per row of head_id (four / eight per lane of the 16-lane row)
 *   head_id  [B][n][head_slots] uint16: slots 0..cnt-1 the head's node ids (any subset of the row; the colony passes the
 *            k largest heuristic entries, ids ascending), the other slots 0, the last slot = cnt (<= head_slots - 1)
 *   paths, flags, dist / costs, nbr, start / fixed_start, seed / iter / iter_offset / ant_gid0 / ant_gid_bstride,
 *   ev_begin / ev_end: as daco_tsp_sample (log-probabilities are not produced: an inference sampler)
 *   stats    optional out [3] uint64 (caller zeroes): dense masked draws (no live head candidate, or after a rejection), tail walks,
 *            rejections; race = 1: stats[0] = steps that took the dense race
 *   workspace  daco_tsp_sparse_workspace_bytes(B, n, A) bytes of device scratch, in this order: the dense rows
 *              P = tau^alpha * eta^beta [B][n][ld] f32 (ld = 512 for n <= 512, else 1024; zeros past n) that the steps which leave
 *              the head walk; the head rows of this iteration (16 lanes x {4 or 8 f32 values, as many u16 ids} per row of tau);
 *              the tours as uint16 [B][A][ld] at daco_tsp_sparse_tours_offset.  Both P and the head rows are written by the pass
 *              over tau of this call, or by daco_pheromone_update_heads.  In the uniform-tail mode (head_eta given, here and there)
 *              the region of P is left alone -- neither written nor read -- and keeps its place.
 *              alpha, beta other than 1: the kernels themselves take unit exponents; tau^alpha and eta^beta are formed first (one
 *              elementwise launch; x^2 = x x and x^0 = 1 exactly) into a workspace of daco_tsp_sparse_workspace_bytes_general(B, n, A)
 *              bytes (= the above + two [B][n][n] f32 matrices), which such a call needs (DACO_E_WORKSPACE otherwise).
 * The switches, for a colony loop that keeps its workspace (tsp/aco.py:75-92 ACO.run: sample -> costs -> best -> update, again
 * and again):
 *   heads_ready  0: the head rows are formed first (one pass over tau and eta);
 *                1: `workspace` already holds this iteration's head rows -- daco_pheromone_update_heads wrote them when it
 *                   finished the rows of tau, for the same tau / eta / alpha / beta / head_id / head_slots / race -- and no
 *                   pass over tau runs.  The caller vouches that tau has not changed since.  Same tours either way.
 *   head_live_max   0, or an upper bound of the live counts in head_id (the k of the colony's head table, <= 62): a launch of
 *                FEW ants (B * ceil(A / 4) <= 256 -- one instance with a few hundred ants, the reference's own call pattern,
 *                tsp/test.ipynb:66-68) then keeps the instance's head rows in LDS when they fit (n <= 512, 64-slot heads,
 *                n * ceil((k + 1) / 4) * 24 bytes <= ~150 KB: TSP-500 with k = 50 does), one wavefront of four ants per
 *                workgroup: the same tours, the per-step L2 round trip gone.  A row with more live slots than the bound sets
 *                bit 2 of flags[b].
 *   nbr_grouped  0: nbr as [B][n][A] (what daco_pheromone_update takes); 1: nbr as [B][ceil(A/8)][n][8] -- the eight ants' entries
 *                of a node together, so that the sampler writes the table in 1 KB pieces instead of 32-byte runs and the update
 *                reads it in runs of R x 32 bytes (daco_pheromone_update_heads(nbr_grouped = 1) takes this form).
 *   dist_symmetric  1: the caller states that every instance of `dist` is bitwise symmetric -- dist[u][v] and dist[v][u] hold the
 *                same bits, which it has checked once for this matrix.  At n <= 512 the fused tour lengths then read each edge
 *                from the upper triangle, dist[min(u, v)][max(u, v)]: the same costs bit for bit from half the cache lines.
 *                0 (and always on a matrix that is not symmetric): every edge is read as dist[u_k][u_{k-1}].
 *   head_eta, tail_c   NULL / 0, or the UNIFORM-TAIL mode, for a heuristic that is one number c outside the head of every row
 *                (what ACO.sparsify writes, tsp/aco.py:52-67: 1e-10 off the k nearest edges): what daco_head_eta wrote for this
 *                eta and head_id, after the caller has read its verdict and found it good.  The same tours, costs, table and
 *                stats, bit for bit.  What differs is the memory touched: the pass over tau (heads_ready = 0) reads tau and
 *                head_eta only and writes the head rows only; the dense-row region of the workspace is neither written nor read;
 *                the rare ways of a step (tail walk, draw without a live head candidate) read the row of tau and multiply by
 *                tail_c, and only the draw after a rejected tail walk reads the rows of tau and eta.  Needs race = 0,
 *                alpha = beta = 1, n % 4 == 0, 16-byte-aligned rows of tau and eta and tail_c >= 0 (DACO_E_BADARG otherwise: the
 *                caller then passes head_eta = NULL; a tail_c without head_eta is refused too).  The head rows a workspace
 *                holds are the same bytes in both modes, the dense rows are not: a caller that leaves the mode runs one call
 *                with heads_ready = 0.
 */
size_t daco_tsp_sparse_workspace_bytes(int B, int n, int A);
size_t daco_tsp_sparse_workspace_bytes_general(int B, int n, int A);
/* daco_tsp_sparse_tours_offset -- where the workspace keeps the tours in their compact form: uint16 [B][A][ld], ld = 512 (n <= 512) or
 * 1024, entry t of ant a = the node visited at step t (entries >= n: undefined).  Valid after a call of
 * daco_tsp_sample_heads with n > 512 (the tours are built there), and for n <= 512 after a call with paths = NULL (nbr or costs given): the
 * colony loop of ACO.run (tsp/aco.py:75-92) keeps `paths` to itself -- costs, best tour and deposit are all it takes from them -- so
 * its iteration asks for no int64 [B][n][A] tensor (131 MB per iteration at TSP-500 x 512 x 64) and hands these rows to
 * daco_track_best (tours16). */
size_t daco_tsp_sparse_tours_offset(int B, int n, int A);
/* daco_tsp_sparse_resident_per_cu -- how many workgroups of the construction kernel a compute unit holds at a time
 * (hipOccupancyMaxActiveBlocksPerMultiprocessor) for the instantiation and the dynamic LDS that daco_tsp_sample_heads
 * launches for these arguments when the launch has more than six and at most eight workgroups of 16 ants per compute unit
 * (another launch of the scan draw on 64-slot heads at n <= 512 has no badly filled second round to remove and keeps whole tours
 * in LDS, six workgroups per compute unit; few ants of one instance take the LDS-heads variant).  The scan draw on 64-slot
 * heads at n <= 512 keeps a 352-entry window of each tour in LDS and parks the first max(0, roundup16(n - 352)) entries in the
 * workspace's tours16 rows (also in a call that returns int64 paths), so that eight workgroups fit: 2 048 workgroups -- TSP-500 x 512
 * ants x 64 instances -- are resident at once on 256 compute units.  0: bad arguments, or the query failed. */
int daco_tsp_sparse_resident_per_cu(int n, int head_slots, int race);
/* daco_tsp_sparse_split_tours -- which launches of the scan draw on 64-slot heads at n <= 512 take the split-tour variant:
 * -1 (default) those with more than six and at most eight workgroups per compute unit, 0 none, 1 all of them (what the tests of the variant and
 * A/B runs set; the tours are the same either way).  Process-wide, not thread-safe against concurrent launches.  Returns the
 * previous mode; any other argument only queries. */
int daco_tsp_sparse_split_tours(int mode);
int daco_tsp_sample_heads(void *stream, int race, int heads_ready, int head_live_max, int nbr_grouped, int dist_symmetric,
                          int B, int n, int A,
                          const float *tau, long tau_bstride, const float *eta, long eta_bstride,
                          float alpha, float beta, const uint16_t *head_id, int head_slots,
                          const int64_t *start, int fixed_start,
                          uint64_t seed, uint64_t iter, const uint64_t *iter_offset, uint32_t ant_gid0,
                          int ant_gid_bstride,
                          int64_t *paths, int32_t *flags,
                          const float *dist, long dist_bstride, float *costs, uint32_t *nbr,
                          unsigned long long *stats,
                          void *workspace, size_t workspace_bytes, void *ev_begin, void *ev_end,
                          const float *head_eta, float tail_c);

/* ---------------------------------------------------------------------------------------------
 * daco_cvrp_sample -- replaces the CVRP ACO.gen_path / pick_move / update_visit_mask /
 * update_capacity_mask / check_done  (cvrp/aco.py:138-205 = cvrp_nls/aco.py:205-272)
 *
 * Node 0 is the depot, n counts the depot.  Every ant starts at the depot and draws from
 * p_k = tau[prev][k]^alpha * eta[prev][k]^beta * visit_mask_k * capacity_mask_k until it is back
 * at the depot with every customer served.  Masks as in the reference: visited customers
 * closed; the depot closed only while the ant stands on it with customers left; candidates with
 * demand_k > capacity - used closed (strict); used resets to 0 at the depot.
 *   demand   [B][n] f32 (demand[0] = 0), capacity scalar
 *   mode     as daco_tsp_sample (DACO_RACE_NOISE: noise [B][noise_steps][A][n], Categorical's
 *            single normalisation)
 *   paths    out [B][Lmax][A] int64; rows past an ant's route are 0 (the reference pads with the
 *            depot until the slowest ant is done); Lmax <= 2n+1 always suffices
 *   logp     out [B][Lmax-1][A] f32 or NULL (padding rows = log(1-eps), as in the reference)
 *   rowsum   out [B][Lmax-1][A] f32 or NULL (with logp): S per draw, for daco_sample_backward
 *   lens     out [B][A] int32 or NULL: rows used by each ant; the reference's L = max(lens)
 *   flags    out [B] int32 or NULL: bit 0 = a draw had no feasible candidate, bit 1 = Lmax or
 *            the noise tensor was too short; caller zeroes it.
 *   dist, costs   optional fusion of gen_path_costs (cvrp/aco.py:133-136): if costs != NULL,
 *            costs [B][A] receives sum_k dist[u_k][u_k+1] over the ant's own route (k ascending).
 *            The reference also adds the (0,0) padding edges of the shorter routes, dist[0][0] =
 *            1e-10 each (cvrp/utils.py): no-ops in f32 for any route longer than 2e-3.
 *   next_table  optional out, daco_directed_table_bytes(B, n, A) bytes: per (node, ant) the node that
 *            follows it plus, per ant, the set of nodes that follow the depot -- the form
 *            daco_pheromone_update(symmetric = 0, nbr = next_table, hub = 0) consumes.
 *   workspace daco_tsp_sample_workspace_bytes(B, n, mode)
 *   demand64, capacity64   NULL / 0, or [B][n] float64 demands and the capacity as a double: the load bookkeeping of
 *            cvrp_nls/aco.py:254-272 (used = used + demand[cur]; demand > capacity - used) then runs in double, as it
 *            does in the reference for that directory's float64 instance data (demands k / capacity: a customer that
 *            fits exactly is common and the last bit decides); `demand` / `capacity` must still be given (their float32
 *            images).  Every layout of the scan draw has the variant (packed kernels for n <= 512, one ant per wavefront above and in the
 *            race modes).
 *   ant_gid_bstride    as in daco_tsp_sample: 0, or the colony's ant count when this call draws a slice [ant_gid0, ant_gid0 + A)
 *            of every colony's ants (ant-sharded colonies keep the single-GPU ant ids)
 *   ev_begin, ev_end   optional hipEvent_t recorded on `stream` right before / after the construction kernel (as in
 *            daco_tsp_sample: the kernel alone, without the weight-matrix kernel and the table memsets before it).
 */
size_t daco_directed_table_bytes(int B, int n, int A);
int daco_cvrp_sample(void *stream, int B, int n, int A,
                     const float *tau, long tau_bstride, const float *eta, long eta_bstride,
                     float alpha, float beta, const float *demand, float capacity, int mode,
                     const float *noise, int noise_steps, uint64_t seed, uint64_t iter,
                     const uint64_t *iter_offset, uint32_t ant_gid0, int ant_gid_bstride, int Lmax, int64_t *paths, float *logp,
                     float *rowsum,
                     int32_t *lens, int32_t *flags,
                     const float *dist, long dist_bstride, float *costs, void *next_table,
                     void *workspace, size_t workspace_bytes, const double *demand64, double capacity64,
                     void *ev_begin, void *ev_end);

/* ---------------------------------------------------------------------------------------------
 * daco_track_best -- replaces the best-so-far bookkeeping inside ACO.run
 *   tsp/aco.py:78-88, cvrp/aco.py:78-100: best_cost, best_idx = costs.min(dim=0);
 *   if best_cost < self.lowest_cost: shortest_path = paths[:, best_idx]; lowest_cost = best_cost
 *   (MMAS: max = n / lowest_cost).  Done on the device, so the loop needs no host branch.
 *   costs [B][A]; paths [B][len][A] int64; lowest [B] f32 in/out (start at +inf); shortest [B][len]
 *   int64 in/out or NULL; best_idx [B] int32 out or NULL (first minimum, torch.min semantics);
 *   mmas_max [B] f32 out or NULL = (1 / lowest) * mmas_scale, the two roundings of the reference's
 *   `problem_size / lowest_cost` on a tensor (reciprocal, then multiply).
 *   tours16, tours_ld   NULL / 0, or the tours in the compact form of daco_tsp_sparse_tours_offset, [B][A][tours_ld] uint16 with
 *   tours_ld >= len (DACO_E_BADARG otherwise): the tour is then read from these rows and `paths` is not; shortest stays int64.
 */
int daco_track_best(void *stream, int B, int len, int A, const float *costs, const int64_t *paths,
                    const uint16_t *tours16, int tours_ld,
                    float *lowest, int64_t *shortest, int32_t *best_idx, float *mmas_max, float mmas_scale);

/* ---------------------------------------------------------------------------------------------
 * daco_prob_matrix + daco_pick_move -- ACO.pick_move as a step-wise service
 *   tsp/aco.py:165-177 and its copies in op/aco.py:186-193, pctsp/aco.py:157-164,
 *   sop/aco.py:156-169, smtwtp/aco.py:139-151, bpp/aco.py:157-164, mkp/aco.py:147-154
 * The sibling problems keep their feasibility rules on the caller's side and only need the
 * draw: dist = tau[prev]^alpha * eta[prev]^beta * mask -> Categorical(dist).sample()/log_prob.
 * daco_prob_matrix builds the fused transition matrix once per solution construction into
 * `workspace` (daco_tsp_sample_workspace_bytes(B, n, mode) bytes); daco_pick_move then performs
 * ONE draw per ant: prev [B][A] int64, mask [B][A][n] f32 (0 = closed), actions out [B][A] int64,
 * logp / rowsum out [B][A] or NULL, noise [B][A][n] for DACO_RACE_NOISE.  `step` keys the Philox
 * counter (use the step index of the construction loop).
 */
int daco_prob_matrix(void *stream, int B, int n, const float *tau, long tau_bstride,
                     const float *eta, long eta_bstride, float alpha, float beta, int mode,
                     void *workspace, size_t workspace_bytes);
int daco_pick_move(void *stream, int B, int n, int A, const void *prob_workspace,
                   size_t workspace_bytes, int mode, const int64_t *prev, const float *mask,
                   const float *noise, uint64_t seed, uint64_t iter, uint32_t ant_gid0, int step,
                   int64_t *actions, float *logp, float *rowsum, int32_t *flags);

/* ---------------------------------------------------------------------------------------------
 * daco_sibling_sample -- fused solution construction for sop / pctsp / op / mkp (one launch)
 *   DACO_SIB_SOP   sop/aco.py:114-180    aux_vec[k] = number of predecessors of k (row sums of
 *                  prec_cons), aux_mat[k][j] = prec_cons[j][k] ("who waits for k"); n-1 draws
 *                  from node 0; paths [B][n][A]; Lmax/lens unused
 *   DACO_SIB_PCTSP pctsp/aco.py:131-188  aux_vec = prizes, scalar0 = min prize; the depot opens
 *                  when the collected prize exceeds scalar0 or nothing is left; ends at the depot
 *   DACO_SIB_OP    op/aco.py:156-224     n counts the dummy end node n-1; aux_mat = distances
 *                  (with the dummy row/column), aux_vec[k] = distances[k][0], scalar0 = max_len;
 *                  a candidate closes for good once route + leg + way home exceeds scalar0
 *   DACO_SIB_MKP   mkp/aco.py:113-183    n counts the dummy item n-1; item_weights [B][n][m],
 *                  scalar0 = capacity (n_items // 2); start [B][A] or NULL (Philox)
 * Variable-length kinds write paths [B][Lmax][A] padded with the resting node (depot 0 / dummy
 * n-1) and lens [B][A]; logp/rowsum [B][rows-1][A] optional; flags as daco_cvrp_sample.  aux_mat
 * is dense [B][n][n] (aux_mat_bstride between instances, 0 = shared).  Draws, modes, noise layout
 * ([B][noise_steps][A][n]) and Philox counters are those of daco_tsp_sample / daco_pick_move.
 * DACO_SIB_SOP draws n - 1 times: its noise_steps must be n - 1 (DACO_E_BADARG otherwise).
 */
#define DACO_SIB_SOP 3
#define DACO_SIB_PCTSP 4
#define DACO_SIB_OP 5
#define DACO_SIB_MKP 6
size_t daco_sibling_workspace_bytes(int B, int n, int mode);
int daco_sibling_sample(void *stream, int kind, int B, int n, int A,
                        const float *tau, long tau_bstride, const float *eta, long eta_bstride,
                        float alpha, float beta, const float *aux_vec, const float *aux_mat,
                        long aux_mat_bstride, float scalar0, const float *item_weights, int m,
                        int mode, const int64_t *start, const float *noise, int noise_steps,
                        uint64_t seed, uint64_t iter, uint32_t ant_gid0, int Lmax,
                        int64_t *paths, float *logp, float *rowsum, int32_t *lens, int32_t *flags,
                        void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * daco_sibling_objective -- objective, elitist key and deposit amount of every ant, for the six sibling problems
 *   (gen_path_costs / gen_sol_obj and the amount update_pheronome adds, of smtwtp/ sop/ pctsp/ op/ mkp/ bpp/aco.py)
 * paths [B][rows][A] int64 as the constructions write them; lens [B][A] int32 or NULL (every ant uses all rows).  Per
 * (instance, ant): obj [B][A] f32 (obj64 [B][A] f64 instead for DACO_SIB_BPP), key [B][A] f32 whose FIRST MINIMUM is the
 * elitist ant (daco_pheromone_update's `costs`), weight [B][A] f32 (its `weights`).
 * The arithmetic is part of the contract: every sum starts at +0.0f (+0.0 for BPP) and is sequential; a multiply and the add
 * that takes it are rounded separately (no fused multiply-add); only an ant's own rows k < lens count.  A node id outside the
 * instance reads as node 0.
 *   DACO_SIB_SMTWTP smtwtp/aco.py:84-111   n = jobs, rows = n + 1 (the nodes daco_tsp_sample(fixed_start = 0) wrote; row 0 is
 *                   the dummy); vec0 = processing_time, vec1 = due_time, vec2 = weights, [B][n] each.  For k = 1..n, j = node - 1:
 *                   t += vec0[j]; late = (t - vec1[j] < 0) ? 0 : t - vec1[j]; c += vec2[j] * late.
 *                   obj = key = c, weight = 1 / (c + 1)
 *   DACO_SIB_SOP    sop/aco.py             mat = distances [B][n][n]; obj = sum_k mat[u_k][u_{k+1}], k ascending: bit for bit
 *                   daco_tour_costs(closed = 0).  key = obj, weight = 1 / obj
 *   DACO_SIB_PCTSP  pctsp/aco.py:104-129   mat = distances, vec0 = penalties [B][n].  length = the open length over the ant's
 *                   rows, k ascending; penalty = sum of vec0[v] over the nodes v not among the ant's rows, v ascending from +0.0f;
 *                   obj = length + penalty, key = -obj (the reference's arg-MAX, pctsp/aco.py:74), weight = 1 / obj
 *   DACO_SIB_OP     op/aco.py:141-147      vec0 = prizes [B][n], n counts the dummy (prize 0); obj = sum_k vec0[u_k], k ascending;
 *                   key = -obj, weight = scale[b] * obj (scale = the colony's Q)
 *   DACO_SIB_MKP    mkp/aco.py             vec0 = prize [B][n] with the dummy item; obj, key, weight as DACO_SIB_OP
 *   DACO_SIB_BPP    bpp/aco.py:26-40,121-126  float64.  vec0 = demand [B][n] f32 (widened exactly), capacity = C.  With
 *                   L = max_a lens[b][a] (the width of the reference's padded matrix; rows without lens), rows past an ant's
 *                   own reading as node 0: for j = 1..L-1: sub += demand[node] if node != 0, else f += (sub / C) * (sub / C),
 *                   sub = 0.  n_bins = L - trailing_zeros - n + 1 (trailing zeros of the padded row; 0 for a row of zeros, as
 *                   count_last_zero has it); cost = -(f / n_bins).  obj64 = cost, key = (float)cost,
 *                   weight = (float)(fit / A), or (float)fit when elitist != 0, with fit = -cost
 * Unused pointers may be NULL.  One launch, one lane per ant, the instance's vectors (and PCTSP's per-lane set of visited nodes)
 * in LDS: 48 KiB at n = DACO_MAX_NODES, DACO_E_TOOLARGE above that.
 *
 * daco_sibling_record -- the record step of the six run() loops on the device, per instance: i = first minimum of key (ties:
 * the lowest ant), and where that ant's objective beats the record under the problem's rule the record and its solution
 * best_sol [B][len - row0] = paths[b][row0..len-1][i] are replaced (an unchanged record leaves best_sol untouched).
 *   rule = the kind.  SMTWTP, SOP: obj < record (start it at +inf);  PCTSP: obj < record (start 1e10; obj is the iteration's
 *   MAXIMUM, sic);  OP, MKP: obj > record (start 0);  BPP: -obj64 > best_obj64 (start 0; best_obj64 holds the fitness).
 *   row0: 1 for SMTWTP (the dummy row is dropped), else 0.  best_idx [B] (optional): i.
 *   mmas_max [B] (optional) is written for every instance from the record AFTER this step:  SOP (1 / record) * mmas_n (two
 *   roundings, as daco_track_best);  PCTSP mmas_n / record (pass n - 1);  OP (record * mmas_n) * mmas_scale[b] (pass the number
 *   of real nodes and Q);  the other rules leave it alone (SMTWTP's bound is 1, MKP's 20: the caller's constants).
 * Both refuse bad input before any launch (DACO_E_BADARG, DACO_E_TOOLARGE for n > DACO_MAX_NODES, daco_last_error()).  The
 * status is the usual DACO_OK / DACO_E_* value typed `long`, for the reason given at daco_rcpsp_net_forward; the refusals are
 * held by tests/test_sibling_objective_spec.py.
 */
#define DACO_SIB_SMTWTP 7
#define DACO_SIB_BPP 8
long daco_sibling_objective(void *stream, int kind, int B, int n, int rows, int A, const int64_t *paths,
                            const int32_t *lens, const float *vec0, const float *vec1, const float *vec2,
                           const float *mat, long mat_bstride, double capacity, int elitist, const float *scale,
                           float *obj, double *obj64, float *key, float *weight);
long daco_sibling_record(void *stream, int rule, int B, int len, int A, const float *key, const float *obj,
                         const double *obj64, const int64_t *paths, int row0, float *best_obj, double *best_obj64,
                        int64_t *best_sol, int32_t *best_idx, float *mmas_max, float mmas_n, const float *mmas_scale);

/* ---------------------------------------------------------------------------------------------
 * daco_reinforce / daco_reinforce_backward -- the REINFORCE tail between a sampler and its backward, one launch each way:
 * the baseline, the masked log-probability sums, the loss of every instance and its gradient (cvrp/train.ipynb:44-49 and
 * the train cells / files of smtwtp, sop, pctsp, op, bpp, mkp, for B instances at once).
 *   obj [B][A] f32 the ants' objectives;  log_probs [B][R][A] f32 as the samplers write them;  lens [B][A] int32 or NULL;
 *   d: the row offset (a sampler whose lens count nodes has lens - 1 draws: d = 1);  sign: +1 minimises, -1 maximises.
 * Forward, per instance b:
 *   live   = R without lens, else max_a lens[b][a] - d clamped to 0..R: the rows the reference's loop produced.  Rows past
 *            it hold the padding's log(1 - 2^-23) and do not count.
 *   s[a]   = sum_{r < live} log_probs[b][r][a]               r ascending
 *   mean   = (sum_a obj[b][a]) / A                            a ascending
 *   adv[a] = sign * (obj[b][a] - mean)                        (the product with +-1 is exact)
 *   loss   = (sum_a adv[a] * s[a]) / A                        a ascending
 * Outputs: loss [B] f32, adv [B][A] f32, live [B] int32.  The batch loss is the mean of loss, the caller's.
 * Backward, given g [B] f32 (d batch loss / d loss[b]), adv and live of the forward:
 *   grad_log_probs[b][r][a] = (g[b] * adv[b][a]) / A for r < live[b], +0.0f for live[b] <= r < R
 * (live outside 0..R is clamped); every one of the B R A words is written, nothing else is.
 * The arithmetic is part of the contract (tests/reinforce_spec.py restates it): every sum starts at +0.0f and is sequential
 * in the order given; a product is rounded before it is added (no fused multiply-add: the library is built with
 * -ffp-contract=off, and the file says so again); the divisions are IEEE, by (float)A.
 * Forward: one workgroup per instance, one lane per ant (strided for A > 256); backward: elementwise over slabs of an
 * instance's R A words.  No atomics, no workspace.  Both refuse a null pointer
 * (lens excepted) and B, A, R <= 0 with DACO_E_BADARG, sign other than +-1 and d < 0 likewise, before any HIP call.  The
 * status is the usual DACO_OK / DACO_E_* value typed `long`, for the reason given at daco_rcpsp_net_forward; the refusals are
 * held by tests/test_reinforce_refusals.py.
 */
long daco_reinforce(void *stream, int B, int R, int A, const float *obj, const float *log_probs, const int32_t *lens, int d,
                    int sign, float *loss, float *adv, int32_t *live);
long daco_reinforce_backward(void *stream, int B, int R, int A, const float *g, const float *adv, const int32_t *live,
                             float *grad_log_probs);

/* ---------------------------------------------------------------------------------------------
 * daco_sibling_backward -- daco_sample_backward for the fused sibling constructions: the gradient of
 * sum(grad_logp * log_probs) w.r.t. eta for solutions drawn by daco_sibling_sample (same kind, aux_vec,
 * aux_mat, scalar0, item_weights; paths / rowsum / lens as that call returned them).  aux_mat is the
 * caller's dense [B][n][n] matrix.  n <= 1024.  grad_eta [B][n][n] is accumulated into (caller zeroes).
 */
int daco_sibling_backward(void *stream, int kind, int B, int n, int A, int rows,
                          const float *tau, long tau_bstride, const float *eta, long eta_bstride,
                          float alpha, float beta, const float *aux_vec, const float *aux_mat,
                          long aux_mat_bstride, float scalar0, const float *item_weights, int m,
                          const int64_t *paths, const float *rowsum, const float *grad_logp,
                          const int32_t *lens, float *grad_eta);

/* ---------------------------------------------------------------------------------------------
 * daco_sample_backward -- replaces autograd through ACO.gen_path(require_prob=True)
 *   (tsp/aco.py:154-176, cvrp/aco.py:153-173; consumed by the REINFORCE losses in
 *    tsp/train.ipynb:45-49, tsp_nls/train.py:31-44, cvrp/train.ipynb:45-51)
 * grad_eta[b][i][k] += sum over draws (t,a) made from node i of
 *     grad_logp[t][a] * beta * ( [k = action] / eta_ik - p_k / (eta_ik * S_ta) ),  0 where the
 * probability was clamped.  rows = n (TSP) or Lmax (CVRP: pass demand, capacity and lens; NULL
 * demand selects TSP).  rowsum is what the sampler wrote.  grad_eta [B][n][n] must be zeroed (or
 * hold a gradient to accumulate into).  f32 hardware atomics: reproducible to rounding.
 * demand64 / capacity64: NULL / 0, or the float64 demands and capacity daco_cvrp_sample drew the routes with (the
 * capacity rule is then replayed in double as well; demand must still be given).
 */
int daco_sample_backward(void *stream, int B, int n, int A, int rows,
                         const float *tau, long tau_bstride, const float *eta, long eta_bstride,
                         float alpha, float beta, const int64_t *paths, const float *rowsum,
                         const float *grad_logp, const int32_t *lens, const float *demand,
                         float capacity, float *grad_eta, const double *demand64, double capacity64);

/* ---------------------------------------------------------------------------------------------
 * daco_tsp_edge_logp / daco_tsp_edge_backward -- the log-probabilities of given TSP tours and their gradient on the k-sparse
 *   graph's EDGE LIST (the training step of tsp/train.ipynb:32-49 and tsp_nls/train.py:15-44 without the [B][n][n] gradient
 *   that daco_sample_backward fills and Net.reshape's backward gathers n k entries of).  The pheromone is ones (every training
 *   step of the reference builds a fresh ACO).
 *   heu [B][E = n k] f32: the network's output; edge j k + t leaves node j (the regular layout daco_tsp_knn_graph writes).
 *   The edges' destinations: exactly one of edge_dst (int64, graph-local ids, [B] rows of E ids edge_dst_bstride elements apart:
 *   row 1 of an edge_index [B][2][E] with stride 2 E) and edge_dst32 (int32 [B][E], ids of the block-diagonal batch graph
 *   b n + local, as daco_tsp_knn_graph_csr's dst32 -- half the bytes).  A destination outside [0, n) is an edge that is never open.
 *   Model: eta_e = heu_e + eps on the graph, eps off it.  At step t from node i: p_e = eta_e^beta over the row's edges whose
 *   destination is unvisited, S = sum p_e + eps^beta (n - t - live neighbours), p_j = the chosen edge's p or eps^beta for a move
 *   off the graph.
 *   daco_tsp_edge_logp:     logp [B][n-1][A] = log clamp(p_j / S, 2^-23, 1 - 2^-23) (the dense kernels' clamp), rowsum [B][n-1][A] = S.
 *   daco_tsp_edge_backward: grad_heu[b][e] += sum over draws (t, a) made from e's row with e live of
 *                           grad_logp[t][a] beta ([e chosen] / eta_e - p_e / (eta_e rowsum[t][a])), nothing for a clamped draw;
 *                           eta = 0 as daco_sample_backward treats it.  The [k = j] term of an off-graph move has no edge and is
 *                           dropped.  grad_heu [B][E] must be zeroed (or hold a gradient to accumulate into).  f32 hardware
 *                           atomics: summation order across ants is not fixed, the result is reproducible to rounding.
 *   Limits: 1 <= k <= 128 (DACO_E_TOOLARGE above), k < n (DACO_E_BADARG), 2 <= n <= DACO_MAX_NODES (DACO_E_TOOLARGE above); every
 *   refusal comes before any HIP call and its daco_last_error() names the dense path, which has none of these limits.  The status is
 *   the usual DACO_OK / DACO_E_* value typed `long`, for the reason given at daco_rcpsp_net_forward.  Added under DACO_VERSION 129:
 *   new entry points only.
 */
long daco_tsp_edge_logp(void *stream, int B, int n, int k, int A, const float *heu, const int64_t *edge_dst,
                        long edge_dst_bstride, const int32_t *edge_dst32, float eps, float beta, const int64_t *paths,
                        float *logp, float *rowsum);
long daco_tsp_edge_backward(void *stream, int B, int n, int k, int A, const float *heu, const int64_t *edge_dst,
                            long edge_dst_bstride, const int32_t *edge_dst32, float eps, float beta, const int64_t *paths,
                            const float *rowsum, const float *grad_logp, float *grad_heu);

/* ---------------------------------------------------------------------------------------------
 * daco_tour_costs -- replaces ACO.gen_path_costs
 *   closed = 1: sum_k dist[u_k][u_{k-1}] over the closed tour     (tsp/aco.py:121-132),
 *               added in the order k = 1..len-1 and the closing edge dist[u_0][u_{len-1}] last
 *   closed = 0: sum_{k < len-1} dist[u_k][u_{k+1}]                  (cvrp/aco.py:133-136)
 * paths [B][len][A] int64, dist [B][n][n] (dist_bstride as above), costs out [B][A] f32.
 * Summation is sequential from +0.0f (documented order; the reference's torch.sum order is
 * unspecified and agreement with it is 1e-5 relative).
 */
int daco_tour_costs(void *stream, int B, int n, int len, int A, const float *dist,
                    long dist_bstride, const int64_t *paths, int closed, float *costs);

/* ---------------------------------------------------------------------------------------------
 * daco_pheromone_update -- replaces ACO.update_pheronome
 *   tsp/aco.py:95-118   (symmetric = 1: both directions of every tour edge, closed tour)
 *   cvrp/aco.py:107-130 (symmetric = 0: directed path[k] -> path[k+1], k < len-1; duplicate
 *                        index pairs of one ant collapse to a single add; floor applied)
 * tau <- tau*decay, then for each ant in index order (elitist = 1: only the first-minimum-cost
 * ant) w = 1/cost and every edge of its tour receives += w; then optional MMAS clamp
 * (clamp_max > 0: tau < clamp_min -> clamp_min, tau > clamp_max -> clamp_max) and optional
 * floor (floor_val > 0: tau < floor_val -> floor_val).  Bit-identical to the reference's
 * sequential loop: each row of tau is owned by one lane-pair and receives its adds in ant
 * order (no atomics).
 *   tau   in/out [B][n][n] f32 (dense, stride n*n)
 *   paths [B][len][A] int64, costs [B][A] f32
 *   clamp_min/clamp_max: [B] f32 device arrays or NULL (per-instance MMAS bounds)
 *   nbr   optional: symmetric: [B][n][A] uint32 as written by daco_tsp_sample; directed: the
 *         next_table written by daco_cvrp_sample (hub must be 0); if NULL it is rebuilt from
 *         `paths` in the workspace
 *   weights optional [B][A] f32: the amount each ant deposits, for the siblings whose rule is
 *         not 1/cost (op/aco.py:134-139 Q*obj, bpp/aco.py:113-118 fit/n_ants, smtwtp/aco.py:90-95
 *         1/(cost+1)); NULL = 1/cost.  `costs` still selects the elitist ant (first minimum).
 *   hub   directed only: the one node a solution may leave several times (depot 0 in cvrp/
 *         pctsp/bpp, the dummy end node in op/mkp); every other node is left at most once;
 *         -1 if there is none (sop, smtwtp).  Edges (hub,hub) of one ant collapse to one add.
 *   workspace: daco_pheromone_update_workspace_bytes(B, n, len, A)
 *   tours16, tours_ld, lowest, shortest   the colony's record kept by the update's own launch; lowest = NULL: not kept (then
 *         shortest and tours16 must be NULL too).  What daco_track_best does -- the first minimum of `costs` (ties: the lowest
 *         index); if it is < lowest[b], lowest[b] and shortest[b][0..n) (int64, or NULL) are replaced -- done by one workgroup per
 *         instance, with the tour read from tours16 ([B][A][tours_ld] uint16, tours_ld >= n) or, tours16 = NULL, from `paths`, which
 *         must then be given.  For the update that uses none of this: elitist = 0, no clamps, symmetric = 1 (else DACO_E_BADARG);
 *         an elitist or MMAS colony calls daco_track_best first.  tau and the record are bit for bit those of the two calls in a row.
 */
size_t daco_pheromone_update_workspace_bytes(int B, int n, int len, int A);
int daco_pheromone_update(void *stream, int B, int n, int len, int A, float *tau,
                          const int64_t *paths, const float *costs, float decay, int elitist,
                          int symmetric, const float *clamp_min, const float *clamp_max,
                          float floor_val, const uint32_t *nbr, const float *weights, int hub,
                          void *workspace, size_t workspace_bytes,
                          const uint16_t *tours16, int tours_ld, float *lowest, int64_t *shortest);

/* daco_pheromone_update_heads -- daco_pheromone_update(symmetric = 1) for a colony whose next construction runs on head rows
 * (tsp/aco.py:95-118 followed by the next iteration's tsp/aco.py:165-172): the workgroup that has just finished rows of tau
 * (evaporation, deposits in ant order, clamp, floor -- bit for bit the update above) also forms their head rows for
 * daco_tsp_sample_heads(heads_ready = 1) from the copy it still holds on chip, so tau is read once per iteration instead of twice.
 *   eta, eta_bstride, alpha, beta, head_id, head_slots, race   as the sampler will be called; alpha = beta = 1 only (other
 *                exponents take the sampler's own pass: DACO_E_BADARG here)
 *   nbr_grouped        the layout of `nbr` (see daco_tsp_sample_heads); a NULL nbr is rebuilt from `paths` either way (paths may be
 *                      NULL when nbr is given: the table is all the deposit reads)
 *   sparse_workspace   the sampler's workspace (daco_tsp_sparse_workspace_bytes(B, n, A)); its head rows are (re)written
 *   head_eta, tail_c   NULL / 0, or the uniform-tail mode as the sampler will be called: the same tau and the same head rows, bit for
 *                      bit, formed from the rows of tau the workgroup holds on chip, head_eta and tail_c.  eta is not read (it may be
 *                      NULL) and the workspace's dense rows are not written (at TSP-500 x 64 instances: 64 MB less read and 65.5 MB
 *                      less written per call).  race = 0, n % 4 == 0, a 16-byte-aligned tau and tail_c >= 0, else DACO_E_BADARG.
 *   tours16, tours_ld, lowest, shortest   the record, as daco_pheromone_update keeps it
 *   129 <= n <= 1024; the other arguments as daco_pheromone_update (len = n, hub unused) */
int daco_pheromone_update_heads(void *stream, int B, int n, int A, float *tau,
                                const int64_t *paths, const float *costs, float decay, int elitist,
                                const float *clamp_min, const float *clamp_max, float floor_val,
                                const uint32_t *nbr, const float *weights, void *workspace, size_t workspace_bytes,
                                const float *eta, long eta_bstride, float alpha, float beta,
                                const uint16_t *head_id, int head_slots, int race, int nbr_grouped,
                                void *sparse_workspace, size_t sparse_workspace_bytes,
                                const float *head_eta, float tail_c,
                                const uint16_t *tours16, int tours_ld, float *lowest, int64_t *shortest);

/* daco_allreduce_delta_tau -- the ant-sharded colony's one data-path collective (every rank builds the deposits
 * of ITS ants, delta-tau [B][n][n] f32 = daco_pheromone_update(decay = 1) onto zeros; the ranks sum them; every rank applies
 * tau <- decay * tau + delta) for hosts without torch.distributed: ncclAllReduce(sum, f32, in place) on `stream` through the
 * RCCL the process holds (resolved at run time; no link-time dependency).  comm: the caller's ncclComm_t (one per rank, created
 * with that same RCCL); count: elements of delta.  The Python host of this package issues the same collective through
 * torch.distributed (deepaco_amd/parallel.py), whose communicators are torch's. */
int daco_allreduce_delta_tau(void *comm, void *stream, float *delta, size_t count);

/* ---------------------------------------------------------------------------------------------
 * daco_two_opt -- replaces batched_two_opt_python / _two_opt_python / two_opt_once
 *   tsp_nls/two_opt.py:6-49
 * Best-improvement 2-opt on every tour until no move improves by more than 1e-6 or
 * max_iterations sweeps were done (the reference's loop, including the final non-improving
 * sweep in the count).  Bit-identical to the reference: same f32 expression order, strict
 * minimum with ties to the first (i,j) in row-major order.
 *   dist   [B][n][n] f32 (dist_bstride as above; need not be symmetric -- the NLS driver also
 *          runs it on the perturbed matrix, tsp_nls/aco.py:230-232,248)
 *   dist_T NULL, or the transposed matrices [B][n][n] (dist itself when it is symmetric): lets the incremental
 *          kernel read d[t[i-1]][t[j]] as a row access of the changed segment's nodes (same values, ~18x less L2
 *          traffic); results do not depend on whether it is given
 *   tours  in/out [B][T][n] uint16, one row per tour (the reference's numpy layout, note: the
 *          transpose of `paths`)
 *   sweeps out [B][T] int32 or NULL: sweeps performed per tour
 */
int daco_two_opt(void *stream, int B, int T, int n, const float *dist, const float *dist_T, long dist_bstride,
                 uint16_t *tours, long max_iterations, int32_t *sweeps);

/* ---------------------------------------------------------------------------------------------
 * daco_two_opt_prepare / daco_two_opt_nbr -- the same search as daco_two_opt (tsp_nls/two_opt.py:6-49: same moves,
 * same tours, same sweep counts, bit for bit), evaluating per sweep only the pairs that can be the reference's strict
 * minimum: for the tour edge (x, y) the nodes v with d[x][v] < d[x][y] + tol and the nodes u with d[u][y] < d[x][y] + tol
 * (tol = 4 ulp(2 max|d|) covers the three f32 roundings of the reference's expression; csrc/daco_two_opt_nbr.hip has
 * the argument).  A few thousand evaluations per sweep instead of n^2/2 once tours are near a local optimum (the
 * perturbation / repair passes of the NLS); more than n^2/2 for tours with many long edges (daco_two_opt_auto chooses).
 *   daco_two_opt_prepare: builds, per instance, the sorted neighbour lists and tolerance ranks of `dist` [B][n][n]
 *          (n <= 1024) into `tables` (daco_two_opt_tables_bytes(B, n) bytes).  Once per matrix.
 *   daco_two_opt_nbr: tables = prepare(dist); tables_T = prepare(transposed dist), or the same pointer when dist is
 *          symmetric.  tours / max_iterations / sweeps as daco_two_opt.
 */
size_t daco_two_opt_tables_bytes(int B, int n);
int daco_two_opt_prepare(void *stream, int B, int n, const float *dist, long dist_bstride, void *tables, size_t tables_bytes);
int daco_two_opt_nbr(void *stream, int B, int T, int n, const float *dist, long dist_bstride, const void *tables,
                     const void *tables_T, uint16_t *tours, long max_iterations, int32_t *sweeps);
/*   daco_two_opt_auto: both kernels on one call, chosen per tour and per phase of its search without a host round
 *          trip (three launches: candidates, dense, candidates): the candidate-list kernel while a tour's lists hold
 *          fewer than ~n^2/6 entries (n^2/10 for a non-symmetric matrix), the dense incremental kernel (daco_two_opt's;
 *          dist_T as there, may be NULL) above, until its running rank sum has fallen under half of that -- tours fresh
 *          from a dense heuristic start dense and finish on the candidate lists; with at most 2048 tours the candidate
 *          kernel keeps them all (and runs 1024 threads per tour below 512 tours).  Same result as either kernel alone.
 *          sweeps [B][T] int32 is REQUIRED here (it carries the per-tour state between the launches).
 */
int daco_two_opt_auto(void *stream, int B, int T, int n, const float *dist, const float *dist_T, long dist_bstride,
                      const void *tables, const void *tables_T, uint16_t *tours, long max_iterations, int32_t *sweeps);

/* ---------------------------------------------------------------------------------------------
 * daco_tsp_nls -- replaces ACO.nls (and, with T_nls = 0, ACO.two_opt) in ONE launch
 *   tsp_nls/aco.py:234-258 over tsp_nls/two_opt.py:6-39
 * Per tour: 2-opt on `dist` (at most max_iterations sweeps); then T_nls rounds of { T_p sweeps of 2-opt on `hdist` (the
 * perturbation matrix 1/(eta/rowmax + 1e-5), tsp_nls/aco.py:230-232), 2-opt on `dist` again, keep the tour if its f32
 * length (daco_tour_costs' summation order) is strictly below the best so far }.  The moves of every pass are the
 * reference's (same candidate rule and pair arithmetic as daco_two_opt_nbr); a sweep re-walks only the candidate lists
 * that the previous move can have changed and reuses the cached minimum of every other list (csrc/daco_nls.hip).
 *   tables / tables_T, htables / htables_T: daco_two_opt_prepare of dist / hdist and of their transposes (the same
 *          pointer when the matrix is symmetric); hdist and its tables may be NULL when T_nls = 0
 *   tours  in/out [B][T][n] uint16: the best tour found
 *   sweeps out [B][T] int32 or NULL: sweeps over all passes;  costs out [B][T] f32 or NULL: length of the returned tour
 *   counters NULL or two uint64 on the device, incremented by: [0] sweeps, [1] list entries walked (bench bookkeeping)
 */
int daco_tsp_nls(void *stream, int B, int T, int n, const float *dist, long dist_bstride, const void *tables,
                 const void *tables_T, const float *hdist, long hdist_bstride, const void *htables, const void *htables_T,
                 uint16_t *tours, long max_iterations, int T_nls, long T_p, int32_t *sweeps, float *costs,
                 unsigned long long *counters);

/* ---------------------------------------------------------------------------------------------
 * daco_gnn_forward -- replaces Net.forward in eval mode
 *   EmbNet.forward tsp/net.py:27-45, MLP/ParNet.forward :59-66,74-75, Net.forward :84-88
 * One graph: n nodes with `feats` input features, E directed edges with one attribute each.
 *   x [n][feats], edge_attr [E], src/dst [E] int32 (edge_index rows), rowptr [n+1] int32 = CSR
 *   offsets of the edges grouped by src, perm [E] int32 = edge ids in that grouped order or NULL
 *   if the edge list is already sorted by src (the reference's kNN graphs are).
 *   params: daco_gnn_param_floats(feats) floats, layout documented in csrc/daco_gnn.hip
 *           (BatchNorm folded to scale/shift from the running statistics -> eval mode only).
 *   heu out [E] f32 in (0,1);  emb out [E][32] or NULL (the edge embedding before the head).
 */
size_t daco_gnn_param_floats(int feats);
size_t daco_gnn_workspace_bytes(int n, int E);
int daco_gnn_forward(void *stream, int n, int E, int feats, const float *x, const int32_t *src,
                     const int32_t *dst, const int32_t *rowptr, const int32_t *perm,
                     const float *edge_attr, const float *params, float *heu, float *emb,
                     void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * daco_gnn_train_forward / daco_gnn_train_backward -- replace Net.forward in TRAINING mode and the backward
 * autograd derives from it
 *   EmbNet.forward tsp/net.py:27-45 with BatchNorm on the statistics of the one graph (:21,24,43-44),
 *   MLP/ParNet.forward :59-75; loss.backward() of tsp_nls/train.py:15-44 as far as the network goes.
 * G equal-sized graphs side by side (n = G * n_g nodes, E = G * E_g edges, graph g owns nodes [g*n_g, (g+1)*n_g) and
 * edges [g*E_g, (g+1)*E_g), node ids already offset): every graph is normalised with its own statistics.
 *   x, src, dst, rowptr, perm, edge_attr   as daco_gnn_forward
 *   params     daco_gnn_param_floats(feats) floats in the layout of csrc/daco_gnn.hip with the BatchNorm slots
 *              holding weight (gamma) and bias (beta) instead of the folded scale / shift
 *   heu        out [E]
 *   stats_out  out [12][2][G][32][2] f32 or NULL: (mean, biased variance) of every BatchNorm (index 0 = edge BN,
 *              1 = node BN of the layer), for the caller's running-statistics update
 *   fixed_stats (forward) NULL, or [12][2][32][2] f32 (mean, variance) per layer and BatchNorm (0 = edge, 1 = node): BatchNorm in
 *              EVALUATION mode -- these running statistics normalise every graph instead of its own batch statistics (a
 *              module in eval() whose output still needs a gradient); (backward) the same fact as a flag: the statistics
 *              were constants, g_z = gamma * rstd * g_y
 *   workspace  daco_gnn_train_workspace_bytes(n, E, G) bytes; the forward leaves the activations the backward needs
 *              there: pass the SAME, untouched block to daco_gnn_train_backward
 *   grad_heu   [E] d loss / d heu;   grad_params out: d loss / d params, same layout as params
 *   rowptr_dst, perm_dst (backward)  CSR of the edges grouped by DESTINATION (offsets [n+1], edge ids [E]) or NULL/NULL
 *              (the backward then builds it in the workspace: count, scan, fill, ids ascending per row).  The node
 *              gradients are CSR row sums of per-edge contributions: fixed order, no float atomics.
 *              perm (backward): as in the forward.
 * No library GEMM is called: the 32x32 linears and their weight gradients run on v_mfma_f32_32x32x2_f32.
 */
size_t daco_gnn_train_workspace_bytes(int n, int E, int G);
int daco_gnn_train_forward(void *stream, int n, int E, int feats, int G, const float *x, const int32_t *src,
                           const int32_t *dst, const int32_t *rowptr, const int32_t *perm, const float *edge_attr,
                           const float *params, float *heu, float *stats_out, const float *fixed_stats, void *workspace,
                           size_t workspace_bytes);
int daco_gnn_train_backward(void *stream, int n, int E, int feats, int G, const float *x, const int32_t *src,
                            const int32_t *dst, const int32_t *rowptr, const int32_t *perm, const int32_t *rowptr_dst,
                            const int32_t *perm_dst, const float *edge_attr, const float *params, const float *heu,
                            const float *grad_heu, float *grad_params, int fixed_stats, void *workspace, size_t workspace_bytes);
/* The same two for G graphs of n_g = n / G nodes each whose EDGE counts differ (sop/: the graph is nonzero(adj)).
 *   edge_off   [G + 1] int32 on the device, the caller's: graph g owns edges [edge_off[g], edge_off[g + 1]), edge_off[0] = 0,
 *              edge_off[G] = E; the graphs are listed one after the other, in any order inside a graph (perm as above), and
 *              every edge of graph g has its source in [g n_g, (g + 1) n_g).  An edge finds its graph as src[e] / n_g.
 * Every graph is normalised with its own statistics over its own edge_off[g + 1] - edge_off[g] edges (stats_out reports the
 * biased variance over that count); the node statistics count n_g rows as before; fixed_stats as above (one table for every
 * graph).  Everything else -- arguments, workspace (daco_gnn_train_workspace_bytes(n, E, G)), launch sequence -- is that of
 * the two entries above, which are these bodies with edge_off = NULL and an edge's graph e / E_g.  n % G != 0, a NULL
 * edge_off: DACO_E_BADARG.  A graph without edges is no training input (its statistics would be 0 / 0; it counts one row).
 * The statuses are the usual DACO_OK / DACO_E_* values typed `long`, for the reason given at daco_rcpsp_net_forward; the
 * refusals are held by tests/test_sop_graph_spec.py.
 */
long daco_gnn_train_forward_ragged(void *stream, int n, int E, int feats, int G, const int32_t *edge_off, const float *x,
                                   const int32_t *src, const int32_t *dst, const int32_t *rowptr, const int32_t *perm,
                                   const float *edge_attr, const float *params, float *heu, float *stats_out,
                                   const float *fixed_stats, void *workspace, size_t workspace_bytes);
long daco_gnn_train_backward_ragged(void *stream, int n, int E, int feats, int G, const int32_t *edge_off, const float *x,
                                    const int32_t *src, const int32_t *dst, const int32_t *rowptr, const int32_t *perm,
                                    const int32_t *rowptr_dst, const int32_t *perm_dst, const float *edge_attr,
                                    const float *params, const float *heu, const float *grad_heu, float *grad_params,
                                    int fixed_stats, void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * daco_cvrp_local_search -- replaces ACO.multiple_swap_star's per-ant CPU tasks
 *   cvrp_nls/aco.py:114-126 (one swapstar() call per ant through a thread pool), cvrp_nls/swapstar.py:240-271
 *   (/tmp-file hand-over) and the entry it calls in the vendored HGS-CVRP (Program/C_Interface.cpp:128-172).
 * A deterministic best-improvement search over relocate / swap / intra-route 2-opt moves (specified in
 * csrc/daco_cvrp_ls.hip, restated in oracle/cvrp_ls.py); HGS's own LocalSearch (third-party, randomised neighbourhood
 * order) is NOT reproduced move for move: results are feasible, never worse, and local optima of these neighbourhoods.
 *   dist     [B][n][n] f32 (dist_bstride elements between instances, 0 = shared); need not be symmetric
 *   demand   [B][n] f32, demand[.][0] = 0;  capacity: vehicle capacity in the same unit
 *   paths    in/out [B][Lmax][A] int64: column (b, a) is ant a's route sequence 0 a b 0 c d 0 ... zero-padded
 *            (the layout of ACO.gen_path, cvrp/aco.py:138-165); rewritten in place without empty routes, with
 *            max_moves = 0 too; a column of depots only comes back unchanged (lens 1, moves 0)
 *   max_moves  moves applied at most per solution (the reference's `count`/`limit`)
 *   lens     out [B][A] int32 or NULL: entries used by each solution (including the closing depot; Lmax + 1 for a
 *            column whose last row holds a customer -- the column then holds the first Lmax entries)
 *   moves    out [B][A] int32 or NULL: moves applied
 */
int daco_cvrp_local_search(void *stream, int B, int n, int A, int Lmax, const float *dist, long dist_bstride,
                           const float *demand, float capacity, int64_t *paths, int max_moves, int32_t *lens,
                           int32_t *moves);

/* ---------------------------------------------------------------------------------------------
 * daco_hgs_prepare / daco_hgs_local_search -- the reference's CVRP local search, ROUTE FOR ROUTE
 *   replaces cvrp_nls/aco.py:114-126 (multiple_swap_star: one swapstar() call per ant through a thread pool),
 *   cvrp_nls/swapstar.py:324-346 (the HGS set-up: demands * 1000, capacity 1000.001, num_vehicles = number of routes),
 *   swapstar.py:187-271 (/tmp-file hand-over) and the entry it binds, HGS-CVRP-main/Program/C_Interface.cpp:128-172
 *   `local_search` -> LocalSearch::run (LocalSearch.cpp:3-103): moves 1-9 (LocalSearch.cpp:134-484) under the
 *   nbGranular-nearest restriction (Params.cpp:77-103), first improvement in the order std::shuffle(std::minstd_rand)
 *   fixes (libstdc++), load penalty 10 * max(0.1, min(1000, maxDist / maxDemand)), float64 throughout.
 *   The reference's ctypes structure (swapstar.py:62-74) is 10 fields of the header's 15 (AlgorithmParameters.h:10-28):
 *   HGS reads useSwapStar beyond it, so the reference RUNS WITHOUT SWAP* and with zero coordinates (Params.cpp:40-54;
 *   the export order of LocalSearch.cpp:756-778 is then the route index order).  That is what these entries compute: the
 *   reference's routes entry for entry (oracle/hgs_ls.c use_swap_star = 0; fixtures tests/golden/g11_*).
 *
 * daco_hgs_prepare: per instance and matrix, what Params derives from the matrix alone: maxDist, the correlated vertices
 *   (nb_granular nearest by (cost, index), made symmetric, ascending), the shuffled node order of LocalSearch.cpp:9 and the
 *   generator state behind it.
 *   matrix  [B][n][n] f64 (bstride elements between instances); node 0 is the depot
 *   tables  out, B * daco_hgs_table_bytes(n, nb_granular) bytes
 * daco_hgs_local_search: nstages (1..3) calls of `local_search` in a row on every solution (cvrp_nls/aco.py:443-448
 *   neural_swapstar is three: distances / limit, heuristic-derived matrix / 10, distances / limit), the routes of a stage
 *   handed to the next as the reference's files do (non-empty routes, in export order).
 *   matrices[s], bstrides[s], tables[s], counts[s]   stage s: its matrix [B][n][n] f64, the tables daco_hgs_prepare made
 *            of it, and `count` (the loop bound of LocalSearch.cpp:17); bstrides[s] = 0: ONE matrix [n][n] (transpose
 *            included) and the one table set made of it, shared by the B instances
 *   matrices_t[s]   the transposed copy of matrices[s] (same stride), or NULL (the array itself may be NULL) for a symmetric
 *            matrix: timeCost[v][u] with u the node being improved is read as row u of the transpose, so that a wavefront's 64
 *            gathers fall on a few cache lines instead of 64 (the same numbers either way)
 *   demand   [B][n] f64 AS HGS GETS THEM (the caller multiplies by 1000, swapstar.py:335), demand[.][0] = 0
 *   capacity 1000.001 in the reference (swapstar.py:337)
 *   paths    in/out [B][Lmax][A] int64: column (b, a) is a zero-separated route sequence (cvrp/aco.py:138-165); rewritten
 *            as cvrp_nls/aco.py:22-33 merge_subroutes lays the result out ("0 c1 .. ck" per route, zero padded)
 *   status   out [B][A] int32 or NULL: 0 searched; 1 a stage was skipped because HGS throws there (distances or demands
 *            out of scale Params.cpp:106-111, fleet too small :112, infeasible input Individual.cpp:70) -- the reference
 *            then keeps that stage's input (swapstar.py:341-345); 2 the column is not a complete solution (left untouched)
 *   stats    out [B][A][4] int32 or NULL: moves applied, loops run, evaluation rounds (one per node and re-evaluation),
 *            watchdog (0; the per-stage step budget, 2^31 - 1 steps, ran out at: 1 a route walk, 2 an evaluation round)
 *   workspace daco_hgs_workspace_bytes(B, n, A, Lmax, nb_granular) bytes
 */
size_t daco_hgs_table_bytes(int n, int nb_granular);
int daco_hgs_prepare(void *stream, int B, int n, const double *matrix, long bstride, int nb_granular, void *tables);
size_t daco_hgs_workspace_bytes(int B, int n, int A, int Lmax, int nb_granular);
int daco_hgs_local_search(void *stream, int B, int n, int A, int Lmax, int nstages, const double *const *matrices,
                          const double *const *matrices_t, const long *bstrides, const void *const *tables, const int *counts, const double *demand,
                          double capacity, int nb_granular, int64_t *paths, int32_t *status, int32_t *stats,
                          void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * daco_hgs_local_search_ss -- the same local search WITH SWAP*, as HGS's sources mean it (opt-in)
 *   What a caller of the reference gets once swapstar.py's CAlgorithmParameters carries all 15 fields of
 *   AlgorithmParameters.h:10-28 and useSwapStar = 1 arrives: on top of everything daco_hgs_local_search replaces,
 *   Params.cpp:40-54 (coordinates and polar angles taken over), the circle sector and barycentre angle of
 *   updateRouteData (LocalSearch.cpp:652-707, CircleSector.h:14-58), the SWAP* phase that ends every loop of
 *   LocalSearch::run (LocalSearch.cpp:77-99), swapStar (:486-573) with preprocessInsertions (:594-615) and
 *   getCheapestInsertSimultRemoval (:575-592), and the export in ascending barycentre angle (:756-778), which is also the
 *   order in which the next stage of a multi-stage call numbers the routes.
 *   Exact: the sector arithmetic (integers), the three-best insertion memory and its tie rule (an equal cost goes behind
 *   the kept entry), the choice of the move (first strict minimum over the pairs in U-major order, then the relocations of
 *   a U, then of a V; applied at <= -MY_EPSILON), every cost as the reference's left-to-right float64 sum
 *   (specification: oracle/hgs_ls.c use_swap_star = 1; fixtures tests/golden/g11_* keys paths_ss1_*).
 *   NOT exact, one quantity: a route's barycentre angle is the device library's double-precision atan2, not libm's.  It is
 *   only ever compared with other routes' barycentre angles, so the export order can differ from the reference's only where
 *   two routes' angles lie within that function's error (a few ulp) of each other.
 *   Arguments as daco_hgs_local_search, then
 *   xy      [B][n][2] f64 coordinates, node 0 the depot
 *   polar   [B][n] int32 Client::polarAngle = posmod((int)(32768. * atan2(y_i - y_0, x_i - x_0) / 3.14159265359))
 *           (Params.cpp:42-47), computed BY THE CALLER with libm's atan2 -- the search branches on these through the sector
 *           tests, so they are an input and not recomputed on the device
 *   workspace daco_hgs_workspace_bytes_ss(B, n, A, Lmax, nb_granular) bytes
 *   stats[..][3] watchdog: 3 the budget ran out inside the SWAP* phase
 *   Errors: DACO_E_BADARG for a null xy or polar (and whatever daco_hgs_local_search refuses), DACO_E_TOOLARGE for n above
 *   16000 (16-bit node ids).  A call whose SWAP* state does not fit next to the matrix in the latency mode's LDS takes the
 *   throughput form.  The status is the usual DACO_OK / DACO_E_* value typed `long`, for the reason given at
 *   daco_rcpsp_net_forward; the refusals are held by tests/test_hgs_swap_star_refusals.py.
 */
size_t daco_hgs_workspace_bytes_ss(int B, int n, int A, int Lmax, int nb_granular);
long daco_hgs_local_search_ss(void *stream, int B, int n, int A, int Lmax, int nstages, const double *const *matrices,
                              const double *const *matrices_t, const long *bstrides, const void *const *tables, const int *counts, const double *demand,
                              double capacity, int nb_granular, int64_t *paths, int32_t *status, int32_t *stats,
                              void *workspace, size_t workspace_bytes, const double *xy, const int32_t *polar);

/* ---------------------------------------------------------------------------------------------
 * daco_tsp_knn_graph -- replaces gen_distance_matrix + gen_pyg_data for a batch of instances
 *   tsp/utils.py:4-36, tsp_nls/utils.py:5-45
 * coords [B][n][2] f32 -> dist [B][n][n] (diagonal = diag, 1e9 in the reference; may be NULL),
 * edge_src / edge_dst [B][n*k] int64 (instance-local node ids; sources sorted, k per node,
 * neighbours by ascending distance, ties -> smaller index) and edge_attr [B][n*k] f32.
 */
int daco_tsp_knn_graph(void *stream, int B, int n, int k, const float *coords, float diag, float *dist,
                       int64_t *edge_src, int64_t *edge_dst, float *edge_attr);
/* The same launch, which also writes the batch as ONE block-diagonal graph in the form daco_gnn_forward takes
 * (src32 / dst32 [B*n*k] int32, node ids b*n + i; the CSR row pointer of it is arange(B*n + 1) * k): what the caller
 * would otherwise derive from edge_src / edge_dst with a handful of elementwise launches per forward. */
int daco_tsp_knn_graph_csr(void *stream, int B, int n, int k, const float *coords, float diag, float *dist,
                           int64_t *edge_src, int64_t *edge_dst, float *edge_attr, int32_t *src32, int32_t *dst32);

/* ---------------------------------------------------------------------------------------------
 * daco_cvrp_knn_graph -- replaces gen_pyg_data of cvrp_nls/utils.py:34-59 for a batch of instances, with the merged CSR
 * B instances of n1 = n + 1 nodes, node 0 the depot.  dist [B][n1][n1] (dist_bstride elements between instances) is the matrix
 * the caller holds: float64 if dist_f64 = 1 (cvrp_nls keeps its instance data in double), float32 if 0; the selection compares
 * its values in their own precision.  Per customer i = 1 .. n the k smallest entries of dist[i][1:] (ascending, ties -> the
 * smaller column; the diagonal's 1e-10 makes every customer its own first neighbour, as torch.topk does in the reference --
 * the self loop is kept), then depot -> i and i -> depot for every customer.  Per instance E = n (k + 2) edges:
 *   edge_index [B][2][E] int64 graph-local ids, edge_attr [B][E] f32 (the matrix entry rounded as .float() rounds it):
 *              edge (i-1) k + r = (i, r-th nearest), n k + (i-1) = (0, i), n k + n + (i-1) = (i, 0), both with dist[i][0]
 *   src32 / dst32 [B E] int32   the batch as ONE block-diagonal graph (ids b n1 + id), in the same edge order
 *   rowptr [B n1 + 1], perm [B E] int32   its CSR by source: perm is the stable argsort by source of the merged edge list (sorted
 *              position -> edge), written in closed form -- the depot has n out-edges, customer i has k + 1:
 *              rowptr[b n1] = b E, rowptr[b n1 + i] = b E + n + (i-1)(k+1); perm[b E + (i-1)] = b E + n k + (i-1),
 *              perm[b E + n + (i-1)(k+1) + r] = b E + (i-1) k + r (r < k), and + k: b E + n k + n + (i-1)
 * Limits: 1 <= k <= n, 2 <= n1 (DACO_E_BADARG), n1 <= DACO_MAX_NODES, B E and B n1 + 1 within int32 (DACO_E_TOOLARGE); every
 * pointer is required.  Refusals come before any HIP call.  The status is the usual DACO_OK / DACO_E_* value typed `long`,
 * for the reason given at daco_rcpsp_net_forward; the refusals are held by tests/test_cvrp_graph_refusals.py.
 */
long daco_cvrp_knn_graph(void *stream, int B, int n1, int k, const void *dist, int dist_f64, long dist_bstride,
                         int64_t *edge_index, float *edge_attr, int32_t *src32, int32_t *dst32, int32_t *rowptr, int32_t *perm);

/* ---------------------------------------------------------------------------------------------
 * daco_sop_graph_count / daco_sop_graph_fill -- replace gen_pyg_data of sop/utils.py:52-57 for a batch of instances
 *   edge_index = nonzero(adj).T, edge_attr = distances[adj.bool()], adj[u][v] = 1 unless u == v or prec[u][v] = 1
 * prec [B][n][n] f32 with 0 / 1 entries (the rows of preceding_mat_gen), dist [B][n][n] f32.  The batch as ONE block-diagonal
 * graph in torch.nonzero's order: instance after instance, source-major, destinations ascending.
 *   count:  rowptr [B n + 1] int32 = the CSR row pointer by source (rows without an out-edge are legal), edge_off [B + 1]
 *           int32 = rowptr[b n]; E = rowptr[B n] is the one word a caller who does not know it reads back to size:
 *   fill:   src32, dst32 [E] int32 global node ids b n + u, edge_attr [E] f32 = dist[b][u][v], cell [E] int64 = the flat index
 *           (b n + u) n + v into [B][n][n].  The pass compares E with rowptr[B n] on the device: if they differ it writes no
 *           edge and sets *bad = 1 (sticky; the caller clears it), so that a wrong E is never an out-of-bounds write.
 * One wavefront per row, a ballot per 64 columns, mbcnt for a lane's slot: no sort, no atomics.
 * Limits: B >= 1, n >= 2, 1 <= E <= B n (n - 1), every pointer (DACO_E_BADARG); B n n < 2^31 (DACO_E_TOOLARGE).  Refusals come
 * before any HIP call; the status is typed `long` as daco_cvrp_knn_graph's, the refusals are held by tests/test_sop_graph_spec.py.
 */
long daco_sop_graph_count(void *stream, int B, int n, const float *prec, int32_t *rowptr, int32_t *edge_off);
long daco_sop_graph_fill(void *stream, int B, int n, int E, const float *prec, const float *dist, const int32_t *rowptr,
                         int32_t *src32, int32_t *dst32, float *edge_attr, int64_t *cell, int32_t *bad);

/* ---------------------------------------------------------------------------------------------
 * daco_heu_matrix -- replaces Net.reshape for a batch, with the "+ eps" its callers add
 *   tsp/net.py:94-102 (matrix = zeros; matrix[edge_index[0], edge_index[1]] = vector), tsp/train.ipynb:35, tsp_nls/test.py:28
 * edge_index [B][2][E] int64 (graph-local ids), heu [B][E] f32 -> out [B][n][n] f32 (16-byte aligned): `fill` everywhere,
 * heu + add at [src][dst] (fill = add = eps gives reshape(...) + eps bit for bit; an edge listed twice: one of its values,
 * as with the reference's indexed assignment).  Ids outside [0, n) are skipped and counted in *bad (may be NULL).
 */
int daco_heu_matrix(void *stream, int B, int n, int E, const int64_t *edge_index, const float *heu, float fill, float add,
                    float *out, int32_t *bad);

/* ---------------------------------------------------------------------------------------------
 * The colony's set-up: daco_sparsify, daco_sparse_head, daco_head_stats (csrc/daco_colony_setup.hip)
 *   ACO.sparsify tsp/aco.py:52-67 (and op/aco.py's, with the prizes as numerator); the head table of the head-row samplers
 *   and the concentration test of sampler='auto' (engine.sparse_head / engine.auto_head_k), which were torch.topk / cumsum /
 *   scatter_ on the device.  One wavefront per matrix row, the row in registers: 2 <= n <= 1024 (DACO_E_TOOLARGE above).
 *   The k-th value of a row comes from a threshold search on the floats' order-preserving integer image; THE TIE RULE of all
 *   three: values compare as floats with -0.0 == +0.0, and of the entries equal to the k-th value the smaller column ids are
 *   taken.  NaN inputs are outside the contract (an unspecified selection; nothing faults).  No host synchronisation.
 *   The statuses are the usual DACO_OK / DACO_E_* values typed `long`, for the reason given at daco_rcpsp_net_forward; the
 *   refusals are held by tests/test_colony_setup_refusals.py.
 *
 * daco_sparsify: dist [B][n][n] f32 (dist_bstride between instances).  Per row the k entries smallest by (value ascending,
 *   column ascending) are selected; out [B][n][n] (dense) = num_j / dist[b][i][j] on the selected columns and num_j / 1e10f on
 *   the others, with IEEE-correct f32 division (bit-equal to torch's `1 / sparse`), the dist value with its own sign of zero.
 *   num_j = 1 if numer is NULL (TSP), else numer[b * numer_bstride + j] (OP's prizes; numer_bstride = 0: one vector for the batch).
 *   Errors: DACO_E_BADARG for k < 1, k > n, n < 2, B < 1, a null dist / out or a negative stride.
 */
long daco_sparsify(void *stream, int B, int n, int k, const float *dist, long dist_bstride, const float *numer,
                  long numer_bstride, float *out);
/* daco_sparse_head: the head table daco_tsp_sample_heads takes (head_id above).  weights [B][n][n] f32 (w_bstride between
 *   instances); per row the k (1 .. 127, <= n) entries largest by (value descending, column ascending), their column ids in
 *   ascending order in slots 0 .. k-1 of ids [B][n][S] uint16, S = 64 for k <= 63, else 128; the other slots 0, slot S-1 = k.
 *   Every slot is written by this call.  w_bstride = 0: one matrix for the batch -- each row is read once and its table
 *   written for all B instances.  Errors: DACO_E_BADARG for k outside 1 .. min(127, n) or a null pointer.
 */
long daco_sparse_head(void *stream, int B, int n, int k, const float *weights, long w_bstride, uint16_t *ids);
/* daco_head_stats: how many rows of weights are concentrated in their K largest entries, for K = 63, 127 and k_lds.
 *   Per row, in float64: tot = the sum of the row, S_K = the sum of its K largest values (= the values above the K-th largest
 *   + the remaining places times that value; K above n counts as n); the row passes K if S_K / tot >= mass (mass_lds for
 *   K = k_lds); a NaN ratio fails.  counts [3] int32 = the passing rows for K = 63, 127, k_lds (integer atomics: the same
 *   on every run); k_lds < 1: not asked, counts[2] = 0.  The rows are those of B matrices, or of the one matrix if w_bstride = 0
 *   (n rows).  The call clears counts itself (a kernel, not a memset node).  Errors: DACO_E_BADARG for a null pointer.
 */
long daco_head_stats(void *stream, int B, int n, const float *weights, long w_bstride, int k_lds, double mass,
                    double mass_lds, int32_t *counts);
/* daco_head_eta: what the uniform-tail mode of the head-row path (daco_tsp_sample_heads, daco_pheromone_update_heads with head_eta)
 *   needs of a heuristic, once per head table.  eta [B][n][n] f32 (eta_bstride between instances, 0: one matrix), head_id
 *   [B][n][head_slots] as daco_sparse_head wrote it (head_slots 64 or 128).
 *   head_eta [B][n][head_slots] f32 = eta at the live slots' ids (slot m < the row's count, id < n), +0 in every other slot.
 *   verdict [3] uint32, cleared by the call (a kernel): verdict[0] != 0 if some row fails on its own -- its entries outside the
 *   head are not all ONE bit pattern, or that pattern has the sign bit set or is not finite, or a live head entry is not >= it;
 *   verdict[1] = max over the rows of ~pattern, verdict[2] = max of pattern.  The mode applies iff verdict[0] == 0 and
 *   ~verdict[1] == verdict[2]; tail_c is then the float with the bits verdict[2].  "One bit pattern" is meant literally: a
 *   tail that mixes +0.0 and -0.0 is refused, and so is a tail of -0.0 (sign bit); +0.0 everywhere is accepted with c = 0.
 *   Errors: DACO_E_BADARG for a null pointer, another head_slots, n < 2; DACO_E_TOOLARGE for n > 1024.
 */
long daco_head_eta(void *stream, int B, int n, const float *eta, long eta_bstride, const uint16_t *head_id, int head_slots,
                   float *head_eta, uint32_t *verdict);

/* ---------------------------------------------------------------------------------------------
 * daco_mkpv_sample -- fused solution construction of the vector-pheromone knapsack colony (one launch)
 *   mkp_transformer/aco.py:111-178 gen_sol / pick_item / update_dummy_state / update_knapsack, with :101-109 gen_sol_obj
 * n counts the dummy item n-1 (n <= 1024, DACO_E_TOOLARGE above).  tau / eta [B][n] f32 are VECTORS over the items
 * (*_bstride between instances, 0 = shared; eta[n-1] is the dummy's 1e-8 of :64): every draw of every ant uses
 * p_k = tau_k^alpha * eta_k^beta * [k open], the first item included (:123-129).  item_weights [B][n][m], 1 <= m <= 8,
 * every capacity is 1 (:7,175): an open item k with any_d(knapsack_d + weight[k][d] > 1) closes for good, strict, float32,
 * knapsack summed in pick order.  An ant whose real items are all closed is done; the reference then draws the dummy with
 * probability 1 until the slowest ant is done, which is the padding written here.
 *   price  [B][n] f32 (price[n-1] = 0) or NULL; with it objs [B][A] = the prices of the picks summed in pick order
 *   mode, noise [B][noise_steps][A][n], seed / iter / ant_gid0: as daco_sibling_sample; draw t = 0, 1, ... is step t + 1
 *   sols   [B][Lmax][A] int64 padded with n-1; lens [B][A] = items of each ant; logp / rowsum [B][Lmax][A] or NULL
 *          (one per draw, log(1 - eps) / 1 in the padding); flags [B] or NULL as daco_cvrp_sample (1: every open candidate had
 *          weight 0, 2: Lmax or the noise tensor too short)
 */
int daco_mkpv_sample(void *stream, int B, int n, int A, int m, const float *tau, long tau_bstride,
                     const float *eta, long eta_bstride, float alpha, float beta,
                     const float *item_weights, const float *price, int mode, const float *noise,
                     int noise_steps, uint64_t seed, uint64_t iter, uint32_t ant_gid0, int Lmax,
                     int64_t *sols, int32_t *lens, float *logp, float *rowsum, float *objs, int32_t *flags);

/* ---------------------------------------------------------------------------------------------
 * daco_mkpv_backward -- replaces autograd through Categorical(dist).log_prob of mkp_transformer/aco.py:141-148
 *   (consumed by the REINFORCE loss of mkp_transformer/train.py:26-30)
 * grad_eta[b][k] += sum over draws (t,a) of grad_logp[t][a] * beta * ( [k = pick] / eta_k - p_k / (eta_k * S_ta) ), 0 where
 * the probability was clamped; sols / rowsum / lens as daco_mkpv_sample returned them, rows = its Lmax.  grad_eta [B][n]
 * is accumulated into (caller zeroes); entries of items no draw had open are not touched; entry n-1 (the dummy) never is.
 * One f32 atomic per (workgroup of four ants, item): reproducible to rounding.
 */
int daco_mkpv_backward(void *stream, int B, int n, int A, int m, int rows, const float *tau, long tau_bstride,
                       const float *eta, long eta_bstride, float alpha, float beta, const float *item_weights,
                       const int64_t *sols, const float *rowsum, const float *grad_logp, const int32_t *lens,
                       float *grad_eta);

/* ---------------------------------------------------------------------------------------------
 * daco_mkpv_update -- mkp_transformer/aco.py:85-99 update_pheronome with the best tracking of run() (:71-83)
 * tau [B][n] in place: tau *= decay; then per ant in index order (elitist != 0: only the first maximum of objs)
 * tau[k] += Q[b] * objs[a] for every item k that occurs in the ant's column of sols [B][rows][A] -- once, however often
 * it occurs (the reference's index-put) -- reading the rows below the longest ant's length (lens [B][A]; NULL: all rows).
 * min_max != 0: every entry below tmin becomes tmin (:98 compares the product (tau > 1e-9) * tau), then every entry above
 * tmax becomes tmax.  Sequential adds in ant order, no atomics on tau: bit-identical to the reference's loop.
 * best_obj [B] (in/out) / best_sol [B][rows] (out) or NULL: where max(objs) > best_obj it replaces it and the ant's column
 * is copied (strict: the first best stays).
 */
int daco_mkpv_update(void *stream, int B, int n, int A, int rows, const int64_t *sols, const int32_t *lens,
                     const float *objs, const float *Q, float decay, int elitist, int min_max, float tmin,
                     float tmax, float *tau, float *best_obj, int64_t *best_sol);

/* ---------------------------------------------------------------------------------------------
 * daco_transformer_forward -- replaces TransformerModel.forward of mkp_transformer/net.py:9-45 without gradients
 *   (mkp_transformer/test.py:14-18): Linear(feats, 32) * sqrt(32), three post-norm encoder layers (d_model 32, 2 heads of
 *   16, softmax over all n keys, d_hid 32, relu, LayerNorm eps 1e-5), ParNet 32-32-32-1 with a sigmoid, heu / heu.max()
 * src [G][n][feats] f32 (G sequences side by side; the reference's batch dimension is 1 per instance) -> out [G][n] f32.
 * params: one flat f32 block of daco_transformer_param_floats(feats) floats (0 for feats outside 1..16) in the layout
 * documented at the top of csrc/daco_transformer.hip (torch's [out][in] matrices in state_dict order of the encoder,
 * the three layers, the decoder); param_floats must equal that count (DACO_E_BADARG).  n <= 4096 (DACO_E_TOOLARGE).
 * workspace: daco_transformer_workspace_bytes(G, n) bytes (DACO_E_WORKSPACE below that).  Nine launches, float32 k-ordered
 * fma chains, no library GEMM, the n x n scores are never written.
 */
size_t daco_transformer_param_floats(int feats);
size_t daco_transformer_workspace_bytes(int G, int n);
int daco_transformer_forward(void *stream, int G, int n, int feats, const float *src, const float *params,
                             size_t param_floats, float *out, void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * daco_transformer_forward_train / daco_transformer_backward -- replace TransformerModel.forward with gradients enabled and
 *   torch autograd through it (mkp_transformer/train.py:15-31, loss.backward()).
 * forward_train: the arithmetic of daco_transformer_forward -- `out` is bit for bit the same -- and what the backward needs in
 * the caller-owned `saved` (daco_transformer_saved_floats(G, n) = 871 G n + 2 G floats; layout in csrc/daco_transformer.h:
 * per layer the input, q/k/v, the attention output, both LayerNorm inputs, the ReLU input; ParNet's hidden rows and the raw
 * sigmoid; the log-sum-exp of every (layer, token, head); every sequence's maximum and the first index attaining it).
 * backward: grad_out [G][n] -> grad_params, daco_transformer_param_floats(feats) floats in the layout of `params`,
 * OVERWRITTEN (no need to clear).  No gradient for src.  src / params / saved as forward_train had / left them.  Flash-style
 * attention backward (the n x n probabilities are recomputed, never written), weight gradients on v_mfma_f32_16x16x4_f32 as
 * per-128-token partials merged in a fixed order: no atomics, no memset, two calls agree bit for bit.  20 launches.
 * workspace: the backward takes daco_transformer_train_workspace_bytes(G, n) bytes of scratch (DACO_E_WORKSPACE below that);
 * forward_train keeps everything in `saved` and needs none: its workspace may be NULL with 0 bytes.  Nothing passes from the
 * forward to the backward but `saved`.  Checks and codes as daco_transformer_forward; a short `saved` is DACO_E_WORKSPACE.
 * Arithmetic: float32, except two float64 accumulators per thread for the softmax row term of the backward.
 */
size_t daco_transformer_saved_floats(int G, int n);
size_t daco_transformer_train_workspace_bytes(int G, int n);
int daco_transformer_forward_train(void *stream, int G, int n, int feats, const float *src, const float *params,
                                   size_t param_floats, float *out, float *saved, size_t saved_floats, void *workspace,
                                   size_t workspace_bytes);
int daco_transformer_backward(void *stream, int G, int n, int feats, const float *src, const float *params,
                              size_t param_floats, const float *saved, size_t saved_floats, const float *grad_out,
                              float *grad_params, void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * daco_rcpsp_* -- the project-scheduling colony of rcpsp/aco.py (Merkle, Middendorf, Schmeck 2002)
 *
 * A project: n activities (0 = source, n-1 = sink), R renewable resources.  Per instance b, dense:
 *   duration [B][n], resources [B][n][R], capacity [B][R], earliest_start / latest_start [B][n], all int32;
 *   succ_ptr [B][n+1] / succ_idx [B][E] int32: the successor lists as CSR (E = entries allocated per instance, the lists of
 *   an instance occupy succ_idx[b][0 .. succ_ptr[b][n]));
 *   horizon: the time slots a usage timeline needs, max(latest_start + duration) over the batch.
 * Limits (DACO_E_TOOLARGE beyond): n <= DACO_RCPSP_MAX_N, R <= DACO_RCPSP_MAX_R, horizon <= DACO_RCPSP_MAX_HORIZON; capacities
 * <= 65535.  The caller vouches that an activity of duration 0 needs no resource (the reference's event queue and the usage
 * timeline used here could part there; deepaco_amd.rcpsp.RCPSPInstance.validate checks it on the host).
 *
 * daco_rcpsp_schedule -- replaces SSGS_ordered (rcpsp/aco.py:42-63) for every ant of update_cost (:222-227)
 *   routes [B][n][A] int64 (activity lists) -> starts [B][n][A] int32 (start time per ACTIVITY; may be NULL) and costs [B][A]
 *   int32 = start of activity n-1.  The reference's rule exactly: start = min(max(first time from the resources' last request
 *   on at which every needed resource has room, ends of the predecessors [earliest_start without any]), latest_start); a
 *   resource with requirement 0 is neither consulted nor advanced; no back-filling before a resource's last request.
 *   flags [B] or NULL (caller zeroes): DACO_RCPSP_FLAG_ORDER = a route is not a topological order of all activities (entries
 *   outside [0, n): that ant is not decoded, cost -1); DACO_RCPSP_FLAG_RESOURCE = a requirement exceeds its capacity, or the
 *   clamp to latest_start broke a resource constraint (the reference raises in request() there), or a time left the horizon.
 *
 * daco_rcpsp_sample -- construct_solutions + update_cost (:176-236) in one call
 *   n-1 draws from activity 0; open = not visited and every direct predecessor visited.  indegree [B][n] f32 and adjacency
 *   [B][n][n] f32 (1 where k is a direct successor of i) are the precedence data in daco_sibling_sample(DACO_SIB_SOP)'s form.
 *   The rule is chosen as the reference chooses it: direct p_k = tau[prev][k]^alpha eta[prev][k]^beta when float(gamma) < 0.05
 *   or c == 1 (then the routes are DACO_SIB_SOP's, draw for draw); otherwise s <- gamma s + tau[prev] (one running vector per
 *   ant) and w_k = (s_k mask_k)^alpha eta[prev][k]^beta, summation p = w when c == 0, balanced p = c p_direct + (1 - c) w
 *   else.  alpha > 0 for those two.  mode, noise [B][n-1][A][n], seed / iter / ant_gid0, logp / rowsum [B][n-1][A] (or NULL):
 *   as daco_sibling_sample.  starts (or NULL), costs, flags as daco_rcpsp_schedule, plus bit 0 of flags (a draw had no
 *   open candidate).  workspace: daco_rcpsp_workspace_bytes(B, n).
 *
 * daco_rcpsp_backward -- gradient of sum(grad_logp * logp) w.r.t. eta for routes drawn by daco_rcpsp_sample with the same
 *   tau / eta / alpha / beta / gamma / c: grad_eta[b][prev][k] += g beta ([k = pick] / eta - w_k / (eta S)), 0 where the
 *   probability was clamped, daco_sample_backward's conventions at eta = 0.  grad_eta [B][n][n] is accumulated into.
 *
 * daco_rcpsp_track -- the record keeping of update_cost (:228-236) and the deposit list of update_pheromone (:242-252)
 *   best_cost [B] int32 in/out (start at INT32_MAX), best_idx [B] int32 in/out, best_route [B][n] int64, best_schedule [B][n]
 *   int32 (or NULL).  alias = 0: best_route is a copy made when the record fell.  alias = 1: the reference's behaviour, whose
 *   best_solution.route is a view of row best_idx of the colony's route tensor and so shows what THAT ANT drew last.
 *   Out, for daco_pheromone_update(len = n, A = C, symmetric = 0, hub = -1, elitist = 0, weights = upd_weights): upd_routes
 *   [B][n][C] int64 and upd_weights [B][C], C = 2 (elitist: best-so-far, iteration best) or A + 1 (best-so-far, every ant);
 *   weights f32(Q / best_cost in float64) and f32(Q) / f32(cost); min_max: clamp_min [B] = tmin, clamp_max [B] = f32(Q n /
 *   best_cost in float64), raised to tmin where below it.
 */
#define DACO_RCPSP_MAX_N 256
#define DACO_RCPSP_MAX_R 8
#define DACO_RCPSP_MAX_HORIZON 8192
#define DACO_RCPSP_FLAG_ORDER 4
#define DACO_RCPSP_FLAG_RESOURCE 8
int daco_rcpsp_schedule(void *stream, int B, int n, int A, int R, int horizon, int E, const int32_t *duration,
                        const int32_t *resources, const int32_t *capacity, const int32_t *earliest_start,
                        const int32_t *latest_start, const int32_t *succ_ptr, const int32_t *succ_idx,
                        const int64_t *routes, int32_t *starts, int32_t *costs, int32_t *flags);
size_t daco_rcpsp_workspace_bytes(int B, int n);
int daco_rcpsp_sample(void *stream, int B, int n, int A, int R, int horizon, int E, const int32_t *duration,
                      const int32_t *resources, const int32_t *capacity, const int32_t *earliest_start,
                      const int32_t *latest_start, const int32_t *succ_ptr, const int32_t *succ_idx,
                      const float *indegree, const float *adjacency, const float *tau, long tau_bstride,
                      const float *eta, long eta_bstride, float alpha, float beta, double gamma, double c, int mode,
                      const float *noise, uint64_t seed, uint64_t iter, uint32_t ant_gid0, int64_t *routes,
                      float *logp, float *rowsum, int32_t *starts, int32_t *costs, int32_t *flags, void *workspace,
                      size_t workspace_bytes);
int daco_rcpsp_backward(void *stream, int B, int n, int A, const float *indegree, const float *adjacency,
                        const float *tau, long tau_bstride, const float *eta, long eta_bstride, float alpha, float beta,
                        double gamma, double c, const int64_t *routes, const float *rowsum, const float *grad_logp,
                        float *grad_eta);
int daco_rcpsp_track(void *stream, int B, int n, int A, const int64_t *routes, const int32_t *starts, const int32_t *costs,
                     double Q, int elitist, int alias, int min_max, float tmin, int32_t *best_cost, int32_t *best_idx,
                     int64_t *best_route, int32_t *best_schedule, int64_t *upd_routes, float *upd_weights,
                     float *clamp_min, float *clamp_max);

/* ---------------------------------------------------------------------------------------------
 * daco_rcpsp_net_forward -- replaces Net.forward of rcpsp/net.py in eval mode, and Net.reshape(...) + eps, for B projects
 *   EmbNet(depth=12, feats=5, edge_feats=2, units=32).forward rcpsp/net.py:30-47, ParNet :72-79, the graph of
 *   RCPSPInstance.to_pyg_data rcpsp/rcpsp_inst.py:202-222 in dense form.
 * B projects of n activities each, ONE launch, one workgroup per project (no cooperative launch, no atomics):
 *   x [B][n][5] f32 node features (duration / max duration, requirements / capacities); feats must be 5 (DACO_E_BADARG)
 *   relation [B][n][n] uint8: 0 = no edge, 1 = precedence edge (attribute [1,0]), 2 = unrelated pair (attribute [0,1]),
 *     3 = the sink's self-loop (attribute [0,0]); edge (i, j) at slot i*n + j; a value above 3 is read as 0
 *   params: daco_rcpsp_net_param_floats() floats, layout at the top of csrc/daco_rcpsp_net.h (that of csrc/daco_gnn.h with 64
 *     floats for e_lin0.weight; BatchNorm folded to scale / shift from the running statistics -> eval mode only)
 *   heu out [B][n][n] f32: sigmoid(logit) + eps on edges, eps exactly elsewhere (Net.reshape's zero plus eps)
 *   logit out [B][n][n] or NULL: the head's pre-sigmoid output on edges, -INFINITY elsewhere
 *   emb out [B][n][n][32] or NULL: the edge embedding before the head on edges, unspecified elsewhere
 *   workspace: daco_rcpsp_net_workspace_bytes(B, n) bytes (0 for B <= 0, n < 2 or n > DACO_RCPSP_NET_MAX_N); its contents
 *     before the call do not matter.  n <= DACO_RCPSP_NET_MAX_N (PSPLIB's largest is 122), DACO_E_TOOLARGE above.
 * Float32 with fixed summation orders: bit-identical from run to run, and a project gives the same bits alone as in a batch.
 * The status is the usual DACO_OK / DACO_E_* value but typed `long`: tests/test_entry_refusals.py demands a row of its own
 * (fixed) table for every export that returns `int`; the refusals of this entry point are held by
 * tests/test_rcpsp_net_refusals.py instead, in that table's form.
 */
#define DACO_RCPSP_NET_MAX_N 128
size_t daco_rcpsp_net_param_floats(void);
size_t daco_rcpsp_net_workspace_bytes(int B, int n);
long daco_rcpsp_net_forward(void *stream, int B, int n, int feats, const float *x, const uint8_t *relation, const float *params,
                            float eps, float *heu, float *logit, float *emb, void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * daco_rcpsp_net_train_forward / _backward -- Net.forward of rcpsp/net.py in TRAINING mode (gnn.BatchNorm normalises every
 * project with its own statistics: the edge BatchNorms over the project's E edges, the node BatchNorms over its n nodes,
 * biased variance, eps 1e-5) and its gradient with respect to the parameters.  Arguments as daco_rcpsp_net_forward, except:
 *   params: the same layout with gamma | beta (not folded scale | shift) in the BatchNorm slots
 *   stats out [12][2 (edge, node)][B][32][2 (mean, biased variance)]: what the running statistics are updated from
 *   saved: daco_rcpsp_net_train_saved_bytes(B, n) bytes the forward fills and the backward only reads (layout at the top of
 *     csrc/daco_rcpsp_net_train.hip; (25 n^2 + 24 n) * 128 + 6144 bytes per project, rounded up to 256: 50.4 MB at n = 128)
 *   grad_heu [B][n][n]: d loss / d heu; entries off the graph are not read
 *   grad_params out: daco_rcpsp_net_param_floats() floats, the sum over the projects in ascending b, d/dgamma and d/dbeta in the
 *     BatchNorm slots; grad_blocks out [B][param_floats] or NULL: every project's own block
 *   workspace (backward): daco_rcpsp_net_train_workspace_bytes(B, n) bytes; contents before the call do not matter
 * One launch per direction, one workgroup per project, plus one small launch that adds the blocks; float64 workgroup sums in
 * a fixed order: bit-identical from call to call, and a project's block is the same alone as in a batch.  Refusals (before any
 * HIP call): bad argument / null pointer DACO_E_BADARG, n > DACO_RCPSP_NET_MAX_N DACO_E_TOOLARGE, short saved or workspace
 * DACO_E_WORKSPACE.  Both size functions give 0 for B <= 0, n < 2 or n > DACO_RCPSP_NET_MAX_N.  The status is a `long`, as
 * daco_rcpsp_net_forward's; its rows are in tests/test_rcpsp_net_train_refusals.py.
 */
size_t daco_rcpsp_net_train_saved_bytes(int B, int n);
size_t daco_rcpsp_net_train_workspace_bytes(int B, int n);
long daco_rcpsp_net_train_forward(void *stream, int B, int n, int feats, const float *x, const uint8_t *relation,
                                  const float *params, float eps, float *heu, float *logit, float *stats, void *saved,
                                  size_t saved_bytes);
long daco_rcpsp_net_train_backward(void *stream, int B, int n, int feats, const float *x, const uint8_t *relation,
                                   const float *params, const void *saved, size_t saved_bytes, const float *grad_heu,
                                   float *grad_params, float *grad_blocks, void *workspace, size_t workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * daco_cvrp_reinsert / daco_cvrp_n1_move / daco_cvrp_adaptive_update -- the "adaptive elitist AS" of cvrp/aco.py:207-383
 *   (improvement_phase, the record of run() :81-93 with intensification_phase / N1_neighbourhood, and update_pheronome |
 *   diversification_phase with the elite pool), one launch each, no host read between them.  Restated in
 *   tests/cvrp_adaptive_spec.py; lane mapping and arithmetic in csrc/daco_cvrp_adaptive.hip and DESIGN.md section 3.20.
 *   dist [B][n][n] f32 (dist_bstride elements between instances, 0 = shared; need not be symmetric; d[0][0] as the instance
 *   has it: it enters the first insertion of every subroute); paths in/out [B][Lmax][A] int64, zero-padded columns
 *   0 a b 0 c 0 0 ... (cvrp/aco.py:138-165); costs in/out [B][A] f32; lens in/out [B][A] int32 or NULL: rows used by a column,
 *   its closing depot included, written for the columns that change.
 *
 * daco_cvrp_reinsert: topk <= 0 or topk >= A selects every ant, anything else the FIVE cheapest (the reference's literal 5,
 *   :342; A < 5 is then DACO_E_BADARG), equal costs at the fifth place going to the smaller ant id.  Each selected ant's
 *   subroutes are rebuilt from [0, 0] by inserting their customers, in their order in the path, at the position of least
 *   (d[p1][c] + d[c][p2]) - d[p1][p2] (float32, left to right, smallest position among equals); the new cost is the double sum
 *   of the subroutes' double sums; the column, its cost (rounded to float32) and length are replaced only if
 *   (float)new < cost.  A column whose last row is a customer keeps that open tail out of the rebuild, as get_subroutes does.
 *   selected out [B][K] int32, K = A or 5: the ants taken, in ascending order of (cost, id) for K = 5.
 *   One workgroup per instance, one wavefront per selected ant (up to 8 at a time, fewer where 64 KiB of LDS hold fewer routes).
 *
 * daco_cvrp_n1_move: one wavefront per instance.  track != 0: first the record -- the first minimum of costs against lowest
 *   [B] (strict <), shortest [B][Lmax] int64 and improved [B] int32 written; track == 0: improved is read, shortest and
 *   lowest are the record as the caller holds it.  Where improved[b] is set, five trials of N1_neighbourhood (:254-286) on the
 *   record: each takes two uniforms u in [0, 1) -- noise [B][5][2] f32, or, noise == NULL, the counter-based stream keyed
 *   by (seed, iter, inst_gid0 + b) -- for the subroute and the node in it, a draw over [lo, hi] being
 *   lo + min(floor(u * (hi - lo + 1)), hi - lo) with the product in float32; route loads are float32 sums in route order,
 *   `load + demand <= capacity` in float32; the candidate is insertion + gain in float32, the running best replaced on strict <
 *   from 0.0.  The best move is applied to shortest and to the record's column of paths (the first minimum of costs), a
 *   subroute left empty disappears, lowest = lowest + delta in float32 is also that column's cost.
 *   mmas_max out [B] or NULL: (1 / lowest) * mmas_scale after the move, for every instance; moved out [B] int32 or NULL.
 *   demand [B][n] f32 (demand[.][0] = 0).
 *
 * daco_cvrp_adaptive_update: per instance, by improved[b].  Set: tau = tau * decay, the first-minimum ant's directed edges
 *   + 1 / cost (each index pair once), clamps, floor -- daco_pheromone_update(elitist = 1, symmetric = 0, hub = 0) bit for bit --
 *   and (shortest[b], lowest[b]) pushed to the front of the instance's pool.  Clear: tau = tau * (decay * 0.5) + 0.01 (the
 *   factor rounded once to float32, multiply and add rounded separately), then + 1 / cost on the edges of every pool entry from
 *   the front; no clamp, no floor.  pool_routes [B][5][Lmax] int64, pool_costs [B][5] f32, pool_state [B][2] int32 =
 *   (entries, slot of the front entry); the entry k places behind the front is slot (front + k) % 5; all three start zeroed.
 *
 * Limits: n <= DACO_MAX_NODES, Lmax <= 4 * DACO_MAX_NODES, A <= 4096 for the reinsertion (DACO_E_TOOLARGE above, before any
 * launch); B, A >= 1, n, Lmax >= 2 and the pointers not marked optional (DACO_E_BADARG).  The statuses are the usual DACO_OK /
 * DACO_E_* values typed `long`, for the reason given at daco_rcpsp_net_forward; the refusals are in
 * tests/test_cvrp_adaptive_refusals.py.  Added under DACO_VERSION 130: new entry points only.
 */
long daco_cvrp_reinsert(void *stream, int B, int n, int A, int Lmax, int topk, const float *dist, long dist_bstride,
                        int64_t *paths, float *costs, int32_t *lens, int32_t *selected);
long daco_cvrp_n1_move(void *stream, int B, int n, int A, int Lmax, const float *dist, long dist_bstride, const float *demand,
                       float capacity, const float *noise, uint64_t seed, uint64_t iter, uint32_t inst_gid0, int64_t *paths,
                       float *costs, int32_t *lens, float *lowest, int64_t *shortest, int32_t *improved, int track,
                       float *mmas_max, float mmas_scale, int32_t *moved);
long daco_cvrp_adaptive_update(void *stream, int B, int n, int A, int Lmax, float *tau, const int64_t *paths, const float *costs,
                               const int32_t *improved, float decay, const float *clamp_min, const float *clamp_max,
                               float floor_val, const int64_t *shortest, const float *lowest, int64_t *pool_routes,
                               float *pool_costs, int32_t *pool_state);

/* ---------------------------------------------------------------------------------------------
 * daco_cvrp_intensify -- the record and the intensification_phase of cvrp_nls/aco.py:419-434: N1_neighbourhood (:313-346) AND
 *   N2_neighbourhood (:348-394) on the record, for B instances in one launch.  Restated in tests/cvrp_nls_adaptive_spec.py;
 *   lane mapping and arithmetic in csrc/daco_cvrp_adaptive.hip and DESIGN.md section 3.21.  The arguments are
 *   daco_cvrp_n1_move's, except: demand [B][n] float32 (demand_f64 == 0) or float64 (!= 0) -- every load (the sequential sum
 *   in route order) and every capacity test runs in that type, capacity rounded to it; noise [B][30] f32 or NULL: entries
 *   2t, 2t+1 are N1's trial t, entries 10 + 4t + k draw k of N2's trial t; without it the counter-based stream keyed by
 *   (seed, iter, inst_gid0 + b, trial), N1's being daco_cvrp_n1_move's draws for the same key and N2's a stream of its own.
 *   N1: as daco_cvrp_n1_move.  N2, trial t, S subroutes (S < 2: the trial is skipped -- the reference raises there):
 *   sr1 = draw(u0, 0, S-1); sr2 = draw(u1, 0, S-2), + 1 if >= sr1; node1 = sr1[draw(u2, 1, len(sr1)-2)]; interior position j
 *   of sr2 is available iff (load[sr2] + d1) - dem[sr2[j]] <= capacity and (load[sr1] - d1) + dem[sr2[j]] <= capacity; none:
 *   no move; else node2 is at the draw(u3, 0, count-1)-th available position; the delta is, one float32 rounding per
 *   operation, ((d[p1,x1] - d[p1,n1]) - d[n1,x1]) + ((d[p2,x2] - d[p2,n2]) - d[n2,x2]), + the least insertion of n1 into sr2
 *   without n2, + that of n2 into sr1 without n1 (smallest position among equals).  The move applied is the first least
 *   delta below 0.0 in the order N1's trials, N2's trials (strict <); lowest = lowest + delta in float32.
 *   moved out [B] int32 or NULL: 0 no move, 1 N1's, 2 N2's.  One workgroup of ten wavefronts per instance, a trial each.
 * Limits: daco_cvrp_n1_move's, and 2 Lmax + (8 | 12) n + 368 <= 65536 bytes of LDS for float32 | float64 demands
 * (DACO_E_TOOLARGE above, before any launch).  A NULL pointer not marked optional is DACO_E_BADARG and the message names it;
 * the refusals are in tests/test_cvrp_nls_adaptive_refusals.py.  Added under DACO_VERSION 130: a new entry point only.
 */
long daco_cvrp_intensify(void *stream, int B, int n, int A, int Lmax, const float *dist, long dist_bstride, const void *demand,
                         int demand_f64, double capacity, const float *noise, uint64_t seed, uint64_t iter, uint32_t inst_gid0,
                         int64_t *paths, float *costs, int32_t *lens, float *lowest, int64_t *shortest, int32_t *improved,
                         int track, float *mmas_max, float mmas_scale, int32_t *moved);

#ifdef __cplusplus
}
#endif
#endif /* DEEPACO_HIP_H */
