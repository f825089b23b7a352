/*
 * frx_debug.h — diagnostics of libfrx.so: traces, in-kernel profiles, self-tests of single kernels.
 *
 * NOT part of the drop-in boundary (include/frx.h is the reference's SE3GCOPTER / cuda_computer boundary plus its neighbours);
 * nothing here is needed to plan a trajectory.  tests/, bench.py and scripts/ use these entries to look inside a plan.
 * Same conventions as frx.h (int status, frx_last_error()).
 */
#ifndef FRX_DEBUG_H
#define FRX_DEBUG_H

#include "frx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic (tests): with FRX_TRACE set in the environment, frx_optimize records for candidate 0 one row per evaluated command
 * {flags, step, f, g.d, gp.d_new, x.x, g.g}; returns the number of rows and copies up to cap_rows of them (7 doubles each). */
int frx_debug_trace(const frx_problem *p, double *out, int cap_rows);
/* Diagnostic: with FRX_RESIDENT_PROF set, the resident kernel runs its instrumented instantiation and leaves 16 counters of 100 MHz
 * ticks per workgroup ([B][G][16], segments RK_P_* of csrc/frx_round_kernel.hpp), then per leader a 16-bin histogram of its waits for a
 * host command ([B][16]: bin k = shorter than 2^k us), then 32 shader-clock stamps of candidate 0's last forward / adjoint bodies;
 * returns the word count, copies up to cap_words. */
int frx_resident_profile(const frx_problem *p, unsigned long long *out, int cap_words);

/* Direction log of the resident round kernel (csrc/frx_round_kernel.hpp).  The kernel computes the L-BFGS direction in the compact
 * (Byrd-Nocedal-Schnabel) form from a register-resident history; the reference computes it with the two-loop recursion
 * (lbfgs.hpp:1381-1411).  frx_debug_direction_log(p, cap_steps, n_cands) makes every later resident plan on the handle record, for the
 * first n_cands candidates and the first cap_steps accepted steps of each, the pair (s, y) the step added to the history, the gradient g
 * the direction was built from and the direction d the cluster returned (cap_steps = 0 switches the log off).
 * frx_debug_direction_log_read copies candidate `cand`'s records: row r = {s[nxp], y[nxp], g[nxp], d[nxp], slot, pair count}
 * (*row_doubles = 4 nxp + 2 doubles, vectors zero-padded from n to nxp); *rows = records written (<= cap_steps); out may be NULL. */
int frx_debug_direction_log(frx_problem *p, int cap_steps, int n_cands);
int frx_debug_direction_log_read(const frx_problem *p, int cand, double *out, int cap_rows, int *rows, int *row_doubles);
/* A candidate that ends with an L-BFGS error on the resident kernel keeps that verdict, like the reference keeps lbfgs_optimize's - except
 * LBFGSERR_INCREASEGRADIENT (a search that starts uphill: only rounding in the compact-form direction can produce it, the two-loop recursion of
 * the per-stage rounds would not), which is planned again on the per-stage rounds by default.  enable = 1: re-run EVERY failed candidate (round 2's
 * behaviour, diagnostic); environment FRX_RESIDENT_RETRY=0|1|t(argeted) overrides.  frx_debug_resident_counts: candidates of the last plan that
 * ended with an L-BFGS error other than the iteration limit on the resident kernel, and how many were re-run. */
int frx_debug_set_resident_retry(frx_problem *p, int enable);
int frx_debug_resident_counts(const frx_problem *p, int *failed, int *retried);
/* Clusters of the last resident plan: = batch size when the batch fitted the chip, fewer when the candidates went through the work queue. */
int frx_debug_resident_clusters(const frx_problem *p, int *clusters);
/* The leader of a cluster runs the host's line-search state machine in step with it and starts on the command it expects (ADVANCE after an
 * accepted trial, or the search's next trial step) before the host's answer arrives; every prediction is checked against the command the
 * host really sent.  out3 = {rounds started on a predicted ADVANCE, rounds started on a predicted trial step, predictions the host's command
 * did not confirm and that were redone} of the last resident plan, summed over the candidates. */
int frx_debug_resident_predictions(const frx_problem *p, unsigned long long *out3);

/* Diagnostic (bench): average microseconds of each stage kernel of an evaluation at x - {forward, penalty, adjoint} - over `reps`
 * back-to-back launches of one kernel at a time, HIP events on the handle's stream. */
int frx_eval_stage_times(frx_problem *p, const double *x, int reps, double *out3_us);
/* One launch per evaluation (fast-racing_amd/csrc/frx_eval_kernel.hpp): frx_objective_eval[_device] run a batch that the chip holds at once - candidates of <= 64
 * pieces, B x (1 + ceil(ceil(N / pieces per wave) / 4)) workgroups <= the device's CU count - as ONE grid of clusters instead of three stage launches, with
 * the same objective bit for bit and the same gradient to <= 1e-10.  set(0) keeps the three launches, set(1) returns to the default, set(2) (tests) is set(1) with members that leave at once, as if
 * they never got a CU, and a 50 us bound on the leader's waits: the evaluation fails with FRX_ERR_TIMEOUT (objective values NaN) and the handle goes on with three launches; frx_debug_eval_fused = workgroups per candidate of the form in use,
 * 0 = one launch per stage.  The environment variable FRX_EVAL_FUSED=0 turns the form off for every handle created afterwards. */
int frx_debug_set_eval_fused(frx_problem *p, int enable);
int frx_debug_eval_fused(const frx_problem *p);
/* Which instantiation of the one-launch form the handle launches: 1 = the compile-time geometry class (17 samples per piece, 3 pieces per wave-task, corridor blocks of 8
 * half-spaces, six reduction steps - the handle's geometry equals it exactly), 0 = the run-time form (any other geometry, FRX_EVAL_GEOM=0, or no one-launch form at all).
 * The two give the same bits. */
int frx_debug_eval_geometry(const frx_problem *p);
/* Which front the handle's one-launch form takes: 1 = two trips behind the entry (the candidate's front record and the argument block's leading lines, then every
 * operand load of the front in one group), 0 = the front that walks the offset tables (FRX_EVAL_FRONT=0, a form without the argument pointer or early durations, or no
 * one-launch form at all).  The two give the same bits. */
int frx_debug_eval_front(const frx_problem *p);
/* Which prelude the forward map of the handle's one-launch form takes: 1 = the shortened one (the axis waves store what they staged without predication, each
 * value at the clamped index it was loaded from, and load it in one basic block), 0 = the form before (FRX_EVAL_PRELUDE=0, a form without the two-trip front or the value-major hand-off, or no one-launch form at all).  The two give the same bits. */
int frx_debug_eval_prelude(const frx_problem *p);
/* Which adjoint the leader of the handle's one-launch form runs: 1 = the one with its operands in front of the poll for the penalty partials (its top reads no offset
 * table - the front's record and lanes hold the values - and an axis lane's waypoint-layer operands and scale factors are requested next to the multipliers), 0 = the
 * form before (FRX_EVAL_ADJOINT=0, a form without the shortened prelude, or no one-launch form at all).  The two give the same bits. */
int frx_debug_eval_adjoint(const frx_problem *p);
/* The solo form of an evaluation (one workgroup per candidate runs forward map, penalty integral and adjoint in ONE launch; batches larger than the clusters of the
 * one-launch form reach; the per-stage rounds of frx_optimize take it too).  mode 0 = never, 1 = from the handle's batch-size threshold on (default; FRX_EVAL_SOLO_MIN_B),
 * 2 = at every batch size, also where the cluster form would apply.  Results are bit-identical to the three stage launches (replaces the same objectiveFunc,
 * se3gcopter_cpu.hpp:961-1000).  frx_debug_eval_solo = workgroups of the kernel a CU holds if the next evaluation takes the form, 0 = it does not. */
int frx_debug_set_eval_solo(frx_problem *p, int mode);
/* which penalty kernel a stage launch of this handle takes: 0 = k_penalty, 1 = k_penalty_lat, 2 = k_penalty_lat2 (large batches: four-wave workgroups, two-phase transpose) */
int frx_debug_penalty_kernel(const frx_problem *p);
int frx_debug_eval_solo(const frx_problem *p);
/* Diagnostic (bench): average microseconds of one evaluation at x in the form frx_objective_eval_device takes, over `reps` back-to-back evaluations. */
int frx_eval_launch_time(frx_problem *p, const double *x, int reps, double *out_us);
/* Diagnostic: one evaluation at x in the one-launch form with shader-clock stamps of candidate 0's cluster: out64[0..12] forward map and [16..31] adjoint as
 * frx_profile_phases, [40..43] the leader's entry / end of the forward map / end of the adjoint / end, [44..48] wave 0 of the first member: entry, gate seen,
 * granules staged, samples done, partials out. */
int frx_debug_profile_eval_cluster(frx_problem *p, const double *x, long long *out64);
/* The same with the stamps of the evaluation's tail behind the first 64 (100 MHz counter, as 40..48): out80[64] wave 0 of the leader behind the barrier that follows
 * the knot adjoint, [65] its last gradient store issued, [66] axis wave 1's last store issued, [67] thread 0 has the verdict, [68] thread 0 has issued `done`;
 * the hand-off of the penalty partials: [69] wave 0 of the first member has the gate word's value, [70] / [71] wave 0 of the leader enters / has left its poll for the
 * partials, [72] / [73] the same for axis wave 1, [74] axis wave 1's Hermite adjoint is done, [75] / [76] NOT times: the spins of lane 0 of wave 0 / of axis wave 1;
 * [77] (frx_debug_eval_adjoint = 1 only, else 0) axis wave 1 has requested its waypoint-layer operands and formed the scale factors, in front of its poll. */
int frx_debug_profile_eval_tail(frx_problem *p, const double *x, long long *out80);
/* The same with the stamps of the forward map's prelude behind those (100 MHz counter).  Wave 0 of the leader, out112[80..84]: at the early barrier, out of it, tau in
 * its register, the coarse durations written, the knot rows built and the first inverse done (the durations formed and the matrix steps: [50], [53..58]); wave 0 of the
 * last member with a task, [88..92]: the same five ([60] its durations formed).  Axis wave 1 of the leader, [96..110]: last staging load issued, out of the early barrier,
 * staging loads landed, staging stores done ([51]: every axis wave has staged), vertex trips done, division done ([52]: waypoint map done and durations seen),
 * right-hand side built, reduction steps 0..5 done, final multipliers seen, coefficients written. */
int frx_debug_profile_eval_forward(frx_problem *p, const double *x, long long *out112);

/* Diagnostic: runs one evaluation at x and returns shader-clock stamps taken at the phase boundaries of candidate 0's
 * k_forward_knot (out32[0..6]) and k_backward_knot (out32[16..24]). */
int frx_profile_phases(frx_problem *p, const double *x, long long *out32);

/* Diagnostic: k_lbfgs_pre (device two-loop recursion) against a host two-loop recursion on random histories, and its
 * duration.  geom4 = {doubles/thread, waves, look-ahead rows, pairs per reduction} or NULL for the library's choice. */
int frx_dv_selftest(int device, int n, int B, int m, int iters, const int *geom4, unsigned seed, double *max_rel_err,
                    double *avg_us);

/* Diagnostic (tests): the layout the device-vector L-BFGS runs with when the longest vector of a batch has n_max elements (csrc/frx_device.hpp, dv_geometry and
 * dv_row_stride themselves): out5 = {doubles/thread E, waves W, look-ahead rows PF, pairs per reduction BLK, row stride hs of the history in doubles}.
 * geom4 = {E, W, PF, BLK} to ask for the row of that geometry, NULL for the library's choice; tight = 0 gives the full row 64 W E.  Needs no device. */
int frx_debug_dv_layout(int n_max, const int *geom4, int tight, int *out5);
/* Diagnostic (tests): ONE round of the device-vector L-BFGS on state the caller owns (host arrays): they are uploaded, k_lbfgs_pre runs the commands
 * cmd[B] (struct DvCommand of csrc/frx_lbfgs.hpp: int flags, slot, bound, newest; double step), k_lbfgs_post follows when f[B] is given, and everything is
 * copied back.  xoff[B+1] delimits the packed vectors x, g, xp, gp, d; S, Y are [B][m][hs], ys [B][m], gt [B][m][4]; res[B] (struct DvResult: 8 doubles f, dg,
 * xx, gg, dginit, 3 unused) goes in and comes out; poff[B+1] with dflags[B] and pflags[poff[B]] are optional (NULL).  lens7 = the lengths, in elements, of
 * {each packed vector, S and Y each, ys, gt, dflags, pflags, res}: an array may be longer than the batch needs, its whole length makes the trip, so a
 * sentinel behind the used part shows a store that went astray.  geom4 and hs as frx_debug_dv_layout gives them for the batch's longest vector (hs tight
 * or full).  Allocates per call; adds no arithmetic. */
int frx_debug_dv_round(int device, int B, int m, const int *geom4, int hs, const long long *lens7, const int *xoff, double *x, double *g, double *xp, double *gp,
                       double *d, double *S, double *Y, double *ys, double *gt, const void *cmd, void *res, const int *poff, int *dflags, int *pflags,
                       const double *f);

/* The jump-point neighbour tables in the reference's storage order (JPS3DNeib ns[27][3][26], f1/f2[27][3][12]; JPS2DNeib
 * ns[9][2][8], f1/f2[9][2][2]; graph_search.h:72-127), generated from rules instead of spelled out; for the parity test. */
int frx_jps_tables(int *ns3, int *f13, int *f23, int *ns2, int *f12, int *f22);

/* Host CPU budget of a resident plan (frx_host_cpus.cpp, host_cpu_share): *budget = CPUs this process may use (affinity mask, cut by the cgroup quota cpu.max);
 * *share = this plan's part of them when LOCAL_WORLD_SIZE ranks of a node (FRX_LOCAL_RANKS overrides) and `extra_plans` further plans of this process
 * (the other shards of a frx_multi job) spin next to it; *mailbox_threads = the service threads a resident plan of `clusters` clusters would start
 * (the caller included): min(one per sixteen clusters, at most four; share - 1), at least one.  FRX_HOST_CPUS overrides the budget (tests). */
int frx_debug_host_cpu_share(int clusters, int extra_plans, double *budget, int *share, int *mailbox_threads);

/* Take-over (frx_optimize.cpp, TakeOver): a batch too large for the resident round kernel runs as per-stage rounds until no more candidates are left than the chip has
 * clusters for; those continue on the resident kernel with their history as it stands.  frx_debug_taken_over: how many candidates of the last plan finished
 * that way (0: none).  frx_debug_compact_from_history: the host code that rebuilds the resident kernel's dense state for such a candidate - R^-1 by slot
 * ([128][129]), Y^T Y ([128][128]), D = diag(s.y) ([128]) - from history rows S, Y [m][hs] (n significant doubles per row), `bound` valid pairs, the newest
 * in slot `newest` (frx_compact.hpp); exported so that a CPU test can check it against a dense inverse.  FRX_TAKEOVER=0 switches take-overs off. */
int frx_debug_taken_over(const frx_problem *p, int *candidates);
/* Tests: rounds > 0 makes every later plan on the handle start as per-stage rounds and hand ALL its running candidates to the resident kernel after that many
 * rounds, whatever the batch size (a small batch would otherwise never take this path); 0 returns to the library's own rule.  (Until round 5 an environment
 * variable read inside frx_optimize did this - and silently switched the resident path off in any process that inherited it.) */
int frx_debug_set_takeover_at(frx_problem *p, long rounds);
int frx_debug_compact_from_history(int m, int n, int hs, int bound, int newest, const double *S, const double *Y, double *rinv129, double *yy, double *vd);

/* Tests: frx_trajectory_clearance splits the cloud into chunks, one workgroup per (piece, chunk), by a rule of its own (fast-racing_amd/csrc/frx_traj_host.hpp,
 * cloud_split).  points > 0 forces that many cloud points per chunk (the last one shorter) for every later clearance call and workspace query on the
 * handle, 0 returns to the library's rule.  Rows do not depend on it. */
int frx_debug_set_clear_chunk(frx_problem *p, int points);

/* Tests: frx_trajectory_clearance_exact splits the cloud into chunks, one one-wave workgroup per (piece, chunk) (fast-racing_amd/csrc/frx_traj_host.hpp,
 * cloud_split), and leaves out the points its cull proves irrelevant.  chunk_points > 0 forces that many cloud points per chunk (the last one shorter)
 * for every later exact clearance call and workspace query on the handle, 0 returns to the library's rule; cull_on == 0 makes every point a survivor that
 * runs both tasks.  Rows depend on neither.
 * frx_debug_clear_exact_counts: per piece (survivors[P], ell_tasks[P]) how many points survived the cull and how many ran the degree-21 task in the last exact
 * clearance call on the handle, summed over the chunks; read from the partials that call left in its workspace, which must still be alive (the blocking form's
 * is the handle's own cloud buffer: a dense frx_trajectory_clearance call on the handle lays it out anew, and the counts are FRX_ERR_INVALID_ARG until the next exact
 * call).  Waits for the device. */
int frx_debug_set_clear_exact(frx_problem *p, int chunk_points, int cull_on);
int frx_debug_clear_exact_counts(frx_problem *p, int *survivors, int *ell_tasks);

/* Tests: the host fold of frx_trajectory_check (kind 0), _extrema (1) and _clearance (2), piece rows to candidate rows and flag words - the code the blocking
 * entries run (fast-racing_amd/csrc/frx_traj_fold.hpp) - on rows the caller supplies: candidate b owns the pieces piece_off[b] .. piece_off[b + 1] - 1 of T[] and
 * rows[] (FRX_CHECK_ / FRX_EXTREMA_ / FRX_CLEAR_FIELDS doubles a piece); limits[4] = {vel_max, thr_acc_min, thr_acc_max, body_rate_max}.  cand_out ([B][fields])
 * and flags ([B]) may each be NULL.  Needs no handle and no device. */
int frx_debug_fold_rows(int kind, int B, const int *piece_off, const double *T, const double *rows, const double *limits, double *cand_out, unsigned *flags);

/* Tests: the sight line of frx_corridor_generate_batch (map_blocked, fast-racing_amd/csrc/frx_chain_kernel.hpp) run on the device for n_pairs pairs of points
 * a[3 n_pairs], b[3 n_pairs] (host buffers; the map's cells are uploaded): out[i] = 0 / 1, to be compared with frx_map_is_blocked verdict for verdict. */
int frx_debug_map_blocked_device(int device, const frx_voxel_map *map, int n_pairs, const double *a, const double *b, int *out);

/* Diagnostic (bench): the shader clock the device sustains under a latency-bound FP64 load (one lone wave per CU on every CU, a dependent FMA chain for `ms`
 * milliseconds): shader cycles per tick of the constant 100 MHz counter, as MHz - minimum, mean and maximum over the CUs' workgroups.  A round of the resident kernel
 * is a chain of dependent instructions: its time is cycles / this clock, which is what differs between the boxes of a pool running the same code object. */
int frx_debug_shader_clock(int device, double ms, double *mhz_min, double *mhz_mean, double *mhz_max);
/* Tests: the neighbour exchange of the one-launch evaluation's reduction steps (lane_exchange<stride>, fast-racing_amd/csrc/frx_wave.hpp) on one wave of the device:
 * in64[64] -> below64[i] = in64[i - stride], above64[i] = in64[i + stride], stride in {1, 2, 4, 8, 16, 32}; 64-bit words moved as they are (host buffers).  A lane
 * without a source lane holds anything. */
int frx_debug_lane_exchange(int device, int stride, const void *in64, void *below64, void *above64);
/* where the resident plan's mailboxes live: out4 = {NUMA node of the command mailbox's page, of the result mailbox's page, the device's NUMA node, the caller's CPU}; -1 = unknown */
int frx_debug_mailbox_numa(const frx_problem *p, int *out4);

#ifdef __cplusplus
}
#endif
#endif /* FRX_DEBUG_H */
