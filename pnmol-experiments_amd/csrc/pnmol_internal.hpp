// Private to the library: what the translation units under csrc/ share.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <string>
#include <vector>

#include "pnmol_cursor_plan.hpp"
#include "pnmol_hip.h"
#include "pnmol_observe_plan.hpp"  // (times_agree lives there: the plan's walk uses it without anything of HIP)

constexpr int NB = 32;    // factorisation block
constexpr int MAXN = 4;   // max derivatives + 1

namespace {
// (unnamed on purpose: kernels of pnmol_hip.hip take it by value and their symbol names spell the namespace)
struct IwpConsts {
    double A1[MAXN * MAXN];  // flip(pascal_lower)  base/iwp.py:24-27
    double Q1[MAXN * MAXN];  // flip(hilbert)       base/iwp.py:29
    double ts[MAXN];         // frame change  s_old[a] / s_new[a]
};
}  // namespace

#define HIPCHK(ctx, call)                                                                        \
    do {                                                                                         \
        hipError_t e__ = (call);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                     \
            return -2;                                                                           \
        }                                                                                        \
    } while (0)

inline int round_up(int x, int q) { return (x + q - 1) / q * q; }

inline double nordsieck_scale(int nu, int a, double dt) {  // base/iwp.py:55-62
    double fact = 1.0;
    for (int q = 2; q <= nu - a; ++q) fact *= q;
    return std::pow(std::fabs(dt), nu - a + 0.5) / fact;
}

struct pnmol_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // Lifetime rule of the C ABI (include/pnmol_hip.h, "Lifetimes"): a handle keeps its parent alive.  `children` counts
    // the live pnmol_filter / pnmol_sqrt_filter objects of this ctx; pnmol_ctx_destroy refuses (-1) while it is not zero.
    std::atomic<int> children{0};
};

// Workspace of one tile sweep (launch_sweep, pnmol_hip.hip) outside the filter step: the matrix G (rt x cb tiles of NB x NB,
// leading dimension ld = cb NB) that the caller fills, the result F of the same shape, the L_jj^-1 tiles, the feed tiles of
// the register-resident kernel, the dependency flags and the info word.
struct SweepWs {
    double *G = nullptr, *F = nullptr, *Linv = nullptr, *feed = nullptr;
    int *flags = nullptr, *info = nullptr;
    int nflags = 0;
    int rt = 0, cb = 0, ld = 0;
    bool left_looking = false;  // this shape runs k_sweep (more than 17 column blocks, or PNMOL_HIP_SWEEP_RL=0), not k_sweep_rl
};
// Allocate for a shape; F and Linv are zeroed on the ctx stream (the sweep never writes all of them).  A tall shape (rt > cb)
// has the error model's layout [...; zero block; I]: G is zeroed and its last cb row blocks are set to the identity.
// On failure nothing is left allocated and the hipError_t is returned.
hipError_t sweep_ws_alloc(SweepWs* w, pnmol_ctx* ctx, int rt, int cb);
void sweep_ws_free(SweepWs* w);
// Zero the flags, reset the info word and launch the sweep of w->G on `st`.  lenient: 0 = a pivot that is not positive is an
// error, 1 = it is dropped (positive semi-definite input).  -1 (ctx->err names `who`): unsupported number of derivatives.
int sweep_ws_enqueue(pnmol_filter* f, const SweepWs& w, hipStream_t st, int lenient, const char* who);
// One reading of a sweep's info word (`limit` = number of pivots): 0, or -2 / -3 with ctx->err = "<who>: <wait>" /
// "<who>: <what> at pivot k".
int sweep_info_result(pnmol_ctx* ctx, int inf, long limit, const char* who, const char* what,
                      const char* wait = "a dependency wait timed out");

// Workspace of a measurement update with qp padded columns (pnmol_state_observe, pnmol_observe.hip): the sweep of the tall matrix
// [S; B; v^T] and one device block [H (qp x dp) | R (qp x qp) | y (qp) | the call's scalars (4)] with the host image of its inputs
struct ObserveWs {
    int qp = 0;
    SweepWs sweep;
    double* dev = nullptr;
    std::vector<double> host;
};

enum class TermKind { none, scalar, system, convection };
// The device image of a term that widens the stencil (pnmol_term_image.hpp): the creation-time operator with a slot for every
// entry the linearisation writes -- w wide; columns, -L's values (0 in an added slot), for a convection term G's value per slot --
// and the (slot_rows, mp) table of the same-point (system) or diagonal (convection) slots.  kind none: no image.
struct TermImage {
    int* col = nullptr;
    double* val = nullptr;
    double* g = nullptr;
    int* slot = nullptr;
    int w = 0, slot_rows = 0;
    TermKind kind = TermKind::none;  // what it was built for
    int ncomp = 0;
};

// one of the filter's per-step tables (LoopTable, pnmol_cursor_plan.hpp) and what the refusal of a call names it and its rows
constexpr int LOOP_TABLES = 3;
struct LoopTableRef {
    LoopTable* tab;
    LoopTableName name;
};

struct pnmol_filter {
    pnmol_ctx* ctx = nullptr;
    int d = 0, n = 0, nu = 0, nB = 0, m = 0, dp = 0, mp = 0, CB = 0, RBS = 0, RBW = 0, RT = 0, ellw = 0;
    int* tickets = nullptr;   // device: read-out blocks that have taken their slot (k_readout with the next step's role)
    int* last_ctr = nullptr;  // device: step-counter value of the last step of the running pnmol_filter_steps call
    int fuse_predict = 1;     // PNMOL_HIP_FUSE_PREDICT: predict the next step's covariance in the down-date epilogue
    int* flags = nullptr;  // k_sweep dependency flags: row[RT], diag[CB], abort, claim[CB*CB] (helpers); k_sweep_rl: rl_flags()
    int nflags = 0;        // words allocated (all of them are zeroed before every sweep)
    double* hs_scratch = nullptr;  // helpers' partial sums, one tile per (row, target step)
    int w_gemm = 0;        // ... and W = (P- H^T) Ls^-T as a GEMM behind a sweep without the rows of W (k_w_gemm)
    int dd_big = 0;        // large problems: sweep alone + k_downdate_big (PNMOL_HIP_DD_BIG=0/1 overrides; see there)
    int sweep_mode = 2;    // PNMOL_HIP_SWEEP: 2 = k_sweep with the covariance down-date riding along in the same launch,
                           // 1 = k_sweep, then k_downdate (any other value: pnmol_filter_create refuses)
    int ds = 0;  // spatial components of the state (= d, or 2d for the latent-force model [u; eps])
    bool counted = false;  // this filter is in live_rl_filters[device]
    bool registered = false;  // this filter is counted in ctx->children
    std::atomic<int> states{0};  // live pnmol_state objects of this filter (pnmol_filter_destroy refuses while > 0)
    int xcd_home = -1;  // k_sweep_rl: >= 0: XCD-local layout (XL), chain workgroup and S row blocks on this XCD; -1: spread layout
    int p32 = 0;        // pnmol_filter_desc.dtype = 1: covariances (state, predicted, Q) are stored and down-dated in fp32
    size_t psz = 8;     // bytes per covariance element
    long Dp = 0;
    IwpConsts iwp{};
    int* ell_col = nullptr;
    double* ell_val = nullptr;
    // the operator given at creation (pde.L), kept for pnmol_filter_set_operator_diagonal: its ELL image, the slot of the
    // diagonal entry of every PDE row (-1: the row has none), and a pinned staging buffer [jdiag d | shift mp]
    int* ell_col_base = nullptr;
    double* ell_val_base = nullptr;
    int* ell_diag_slot = nullptr;
    int base_w = 0, base_has_diag = 0;
    int op_replaced = 0;      // pnmol_filter_set_operator / _set_operator_diagonal have replaced the creation-time operator or shift
    int ell_is_base = 1;      // ell_col / ell_val hold the base image (diagonal slots aside): no dense upload since the last restore
    double* h_op = nullptr;
    double* h_op_dev = nullptr;
    hipEvent_t ev_op = nullptr;
    double *Kg = nullptr, *rdiag = nullptr, *Rdense = nullptr, *shift = nullptr;
    double *G = nullptr, *F = nullptr, *Linv = nullptr, *Ppred = nullptr, *mpred = nullptr, *zbuf = nullptr;
    double *var = nullptr, *Sqinv = nullptr, *rec = nullptr, *part = nullptr;
    int* info = nullptr;
    std::vector<double> sqdiag;
    double* Qfull = nullptr;  // Q1 (x) K as a dense Dp x Dp matrix (on-device error model), allocated on first use
    int* one = nullptr;       // device constant 1 (step-counter stand-in for sweeps outside the step loop)
    int* info_err = nullptr;  // info word of those sweeps
    double sq_dt = -1.0;
    std::vector<double> hB;   // host copy of pde.B (nB x d) for operator rebuilds
    int ell_cap = 0;          // allocated ELL width
    // scratch state for ping-pong inside steps()
    double *tmpP = nullptr, *tmpMean = nullptr;
    double *rec_means = nullptr, *rec_stds = nullptr;
    double* h_pin = nullptr;  // pinned host staging: [rec 4k | means k*d | stds k*d | info k ints]
    double* h_pin_dev = nullptr;  // the same buffer as the device sees it (mapped)
    int rec_cap = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.f;
    int* ctr = nullptr;  // device step counter (slot of the per-step outputs)
    int pending_k = 0;   // steps enqueued by pnmol_filter_steps_begin and not yet collected
    double pending_dt = 0.0;
    pnmol_state* pending_state = nullptr;
    struct GraphEntry {
        double *P0, *P1, *var;
        double dt;
        int nsteps;
        bool have_sq;
        bool fused;
        hipGraphExec_t exec;
        bool launched;  // the first launch of an executable graph costs ~50 ms of host time (ROCm 7.2)
    };
    std::vector<GraphEntry> graphs;
    int graph_chunk = 10;  // steps per captured graph (even); 0 disables graphs
    // RTS smoother (pnmol_smoother_step), allocated on first use: the sweep's tall matrices [P-; P A^T; 0; I] -> [L; V; 0; T]
    // ((3 Dp/32 + 1) * 32 x Dp), its L_jj^-1 tiles, feed tiles and flags, and G, C, Ps^h (Dp x Dp), [m^h | dm] (2 Dp)
    SweepWs sm_sweep;
    double *sm_gain = nullptr, *sm_C = nullptr, *sm_Psh = nullptr, *sm_vec = nullptr;
    // The whole backward pass in one call (pnmol_smoother_steps), allocated on its first use: two states' worth of buffers
    // ([P | mean | var], Dp^2 + 2 Dp doubles each) that a pass without `out` rotates, the device read-out [means | stds] of
    // sm_ro_rows rows of d with the per-step info words behind them, and its pinned host image
    double* sm_rot[2] = {nullptr, nullptr};
    double *sm_ro = nullptr, *sm_ro_pin = nullptr;
    int sm_ro_rows = 0;
    // Joint draws (pnmol_samples_*), allocated on first use: the square lenient sweep P^h -> C (sp_Gc, sp_F: Dp x Dp, its
    // L_jj^-1 tiles, feed tiles, flags, info word), Gamma (dp x dp, from the host copy kept at creation) and m^h (Dp).  The
    // main sweep of a backward step runs in the smoother's workspace above.
    SweepWs sp_sweep;
    double *sp_Gamma = nullptr, *sp_mh = nullptr;
    // a backward step has two independent sweeps (P^h -> C and [P-; P A^T; 0; I]): on wide problems the second one runs on
    // this side stream, between the two events, while the ctx stream factorises P^h and forms xt and r
    hipStream_t sp_stream = nullptr;
    hipEvent_t sp_ev_built = nullptr, sp_ev_swept = nullptr;
    std::vector<double> hGamma;        // desc->Gamma padded to dp x dp (white-noise fp64 filters)
    std::atomic<int> samples{0};       // live pnmol_samples objects of this filter (pnmol_filter_destroy refuses while > 0)
    // Dense output (pnmol_bridge_*, pnmol_state_predict_marginals): scratch for the query table and the read-out, grown on demand
    std::atomic<int> bridges{0};       // live pnmol_bridge objects of this filter (pnmol_filter_destroy refuses while > 0)
    void* dn_scratch = nullptr;
    size_t dn_cap = 0;
    struct BridgeSlab* dn_slab = nullptr;  // the slab new bridges take their block from
    // Measurement updates (pnmol_state_observe): one workspace per padded column count, allocated on first use
    std::vector<ObserveWs*> ob_ws;
    // Sensor data in the constant-step loop (pnmol_filter_set_observations, pnmol_observe.hip): NULL = no plan
    struct ObservePlanDev* ob_plan = nullptr;
    // The recorder of the constant-step loop (pnmol_filter_set_recorder, pnmol_record.hip): NULL = none.  While one is set the
    // loop runs non-fused (the fused steady-state launch never writes the posterior covariance) and copies the state behind
    // every step into the next slot
    struct RecordDev* rec_plan = nullptr;
    // The nonlinear term the device linearises itself (pnmol_reaction.hip): none, a pointwise reaction (pnmol_filter_set_reaction),
    // a coupled system (pnmol_filter_set_reaction_system) or a convection term (pnmol_filter_set_convection), with the descriptor of
    // that kind.  While one is set the constant-step loop re-linearises in front of every step, runs non-fused and carries no error
    // model.  `term` changes at the end of a setter that succeeded; a setter that fails leaves TermKind::none on the base operator.
    TermKind term = TermKind::none;
    pnmol_reaction reaction{};
    pnmol_reaction_system sys{};
    pnmol_convection cv{};
    // A filter holds one term, so it owns one image.  A system set again with the same ncomp reuses it (clearing and a scalar
    // reaction leave it alone); a convection term rebuilds it with every set call (G comes with the term), and so does a system set
    // after a convection term -- one more cold setter call than when each kind kept an image of its own.
    TermImage term_img;
    // Driven problems (pnmol_filter_set_forcing, pnmol_filter_force_at, pnmol_forcing.hip): NULL = none.  A forced step reads its
    // shift from a buffer of the forcing's own, so `shift` stays what the operator setters and the term kernels made it.
    struct ForcingDev* forcing = nullptr;
    // A time-dependent operator M(t) = sum_r a_r(t) L_r (pnmol_filter_set_operator_family, pnmol_operator.hip): NULL = none.  While
    // a family is set ell_col / ell_val hold its union image, the operator setters and the terms with an image of their own refuse,
    // and a pointwise reaction linearises on the family's current operator.
    struct OperatorDev* op_family = nullptr;
    // The per-step tables of the constant-step loop (pnmol_loop_table.hip): while one is set the i-th step taken since consumes its
    // row i.  lin_points (pnmol_filter_set_linearization_points): the step is linearised at the row instead of its own predicted
    // mean; the table belongs to the term and goes with it.  forcing_rows (pnmol_filter_set_forcing): the step measures against
    // the row.  op_schedule (pnmol_filter_set_operator_schedule): the step runs with the operator of the row's coefficients; the
    // table belongs to the family and goes with it.  With forcing_rows or op_schedule set the loop runs non-fused, with op_schedule
    // also without an error model.  loop_tables: all of them, in the order in which pnmol_filter_steps_begin refuses.
    LoopTable lin_points, forcing_rows, op_schedule;
    const LoopTableRef loop_tables[LOOP_TABLES] = {
        {&lin_points, LOOP_POINTS}, {&forcing_rows, LOOP_FORCING}, {&op_schedule, LOOP_SCHEDULE}};
    // Linear functionals of the trajectory (pnmol_functionals, pnmol_functional.hip): the workspace of the pass, allocated on first use
    struct FunctionalWs* fn_ws = nullptr;
};
inline bool has_term(const pnmol_filter* f) { return f->term != TermKind::none; }

struct pnmol_state {
    pnmol_filter* f = nullptr;
    double* mean = nullptr;  // Dp
    double* P = nullptr;     // Dp*Dp
    double* var = nullptr;   // Dp   marginal variances, same frame as P
    double t = 0.0;
    double frame_dt = 0.0;  // 0 = raw coordinates, else Nordsieck frame of that dt
};

// The blocks of a filter's bridges come out of slabs of BRIDGE_SLAB_SLOTS blocks: smooth() makes one bridge per step, and a device
// allocation per step is what the bridges would otherwise cost most.  A slab is freed when the last bridge in it is destroyed (the
// filter's current slab is reused instead while it has free slots).
constexpr int BRIDGE_SLAB_SLOTS = 64;
struct BridgeSlab {
    double* base = nullptr;
    int used = 0;  // slots handed out
    int live = 0;  // bridges alive
};

struct pnmol_bridge {
    pnmol_filter* f = nullptr;
    BridgeSlab* slab = nullptr;
    double* blk = nullptr;    // point-diagonal blocks of Ps_k, C_k, Ps_{k+1}, the two means, diag K (pnmol_dense_block_doubles): a slot of slab
    double* Cfull = nullptr;  // C_k (Dp x Dp), kept on request
    double t = 0.0, dt = 0.0; // the interval [t, t + dt]; everything above is in the Nordsieck frame of dt
};

struct pnmol_samples {
    pnmol_filter* f = nullptr;
    int S = 0, Sp = 0;       // draws, padded to a multiple of 64
    double* X = nullptr;     // Dp x Sp: the draws at time t, in the frame frame_dt
    double* Xi = nullptr;    // 2 Dp x Sp: noise [xi_1; xi_2]
    double* Xt = nullptr;    // Dp x Sp: xt = m + s C xi_1
    double* R = nullptr;     // Dp x Sp: Gamma xi_2 per derivative block, then T^T r
    double* Y = nullptr;     // Dp x Sp: r
    double* stage = nullptr; // S x 2D: host-supplied noise / read-out, allocated on first use
    double t = 0.0, frame_dt = 0.0;
    bool drawn = false;
};

// raw-coordinate scale of every derivative in the Nordsieck frame of frame_dt (0 = raw coordinates already)
inline void frame_scales(const pnmol_filter* f, double frame_dt, double* sc) {
    for (int a = 0; a < f->n; ++a) sc[a] = frame_dt == 0.0 ? 1.0 : nordsieck_scale(f->nu, a, frame_dt);
}
inline void frame_scales(const pnmol_state* s, double* sc) { frame_scales(s->f, s->frame_dt, sc); }
// frame change of derivative a from the Nordsieck frame of from_dt (0 = raw coordinates) into that of to_dt
inline double frame_ratio(const pnmol_filter* f, int a, double from_dt, double to_dt) {
    return (from_dt == 0.0 ? 1.0 : nordsieck_scale(f->nu, a, from_dt)) / nordsieck_scale(f->nu, a, to_dt);
}
// lower Cholesky factor of the leading n x n block of A (row pitch MAXN; L zero on entry).  semidefinite: a pivot that is
// not positive gives a zero column instead of a NaN.
inline void small_cholesky(int n, const double* A, double* L, bool semidefinite = false) {
    for (int a = 0; a < n; ++a)
        for (int b = 0; b <= a; ++b) {
            double v = A[a * MAXN + b];
            for (int e = 0; e < b; ++e) v -= L[a * MAXN + e] * L[b * MAXN + e];
            if (!semidefinite) L[a * MAXN + b] = (a == b) ? std::sqrt(v) : v / L[b * MAXN + b];
            else if (a == b) L[a * MAXN + a] = v > 0.0 ? std::sqrt(v) : 0.0;
            else L[a * MAXN + b] = L[b * MAXN + b] > 0.0 ? v / L[b * MAXN + b] : 0.0;
        }
}

// What each feature hung on the filter (pnmol_filter_destroy)
void pnmol_smooth_free_ws(pnmol_filter* f);
void pnmol_sample_free_ws(pnmol_filter* f);
void pnmol_dense_free_ws(pnmol_filter* f);
void pnmol_observe_free_ws(pnmol_filter* f);
void pnmol_functional_free_ws(pnmol_filter* f);
// pnmol_smooth.hip: the smoother's workspace, allocated on first use (a backward sampling step runs its main sweep there)
int pnmol_smooth_ensure_ws(pnmol_filter* f);

// pnmol_observe.hip: the sensor plan inside pnmol_filter_steps_begin / _end.  pending: a plan with entries that have not been applied
// is set (the loop then runs non-fused: the fused loop prepares the next step's z and G from the unconditioned state).
bool pnmol_observe_plan_pending(const pnmol_filter* f);
// the walk of a call of k steps of dt from s (refusals: -1, ctx->err set, nothing enqueued); entry_of_step[j] >= 0: an update
// goes behind step j.  Without a pending plan: all -1.
int pnmol_observe_plan_begin(pnmol_filter* f, const pnmol_state* s, int k, double dt, std::vector<int>* entry_of_step);
// enqueue the update of `entry` on the state (P, mean, var in the frame frame_dt), in place, on the ctx stream; rec_slot >= 0: the
// step record of that slot is overwritten from the conditioned state.  No synchronisation.
int pnmol_observe_plan_enqueue(pnmol_filter* f, int entry, double* P, double* mean, double* var, double frame_dt, int rec_slot);
// behind the call's synchronisation: results of the call's entries from the staging buffer, the cursor moves.  0, or -2 / -3 with
// *step = the step whose update failed (ctx->err names entry and pivot)
int pnmol_observe_plan_collect(pnmol_filter* f, int* step);
// the device result slots the running call fills and where they go (mapped staging): the loop's copy-out kernel carries them home.
// NULL: the call applies no entry.
const double* pnmol_observe_plan_results_dev(const pnmol_filter* f, double** host_dev, int* first, int* count);
// drop the bookkeeping of a call that was refused or failed before it was enqueued in full
void pnmol_observe_plan_abandon(pnmol_filter* f);
// the cursor, and putting it back (pnmol_filter_prepare_steps rehearses a call): entries from `next` on count as not applied again
int pnmol_observe_plan_cursor(const pnmol_filter* f);
void pnmol_observe_plan_rewind(pnmol_filter* f, int next);
void pnmol_observe_plan_free(pnmol_filter* f);

// pnmol_record.hip: the recorder inside pnmol_filter_steps_begin / _end.  active: a recorder is set (the loop then runs non-fused).
bool pnmol_record_active(const pnmol_filter* f);
// s is a slot of the recorder its filter has set (pnmol_state_destroy refuses it)
bool pnmol_record_holds(const pnmol_state* s);
// the refusals of a call of k steps that advances s (-1, ctx->err set; nothing of HIP is touched)
int pnmol_record_begin(pnmol_filter* f, const pnmol_state* s, int k);
// the cursor word of the running call, on the ctx stream (once per call, in front of its steps)
int pnmol_record_enqueue_cursor(pnmol_filter* f);
// k_record behind a step (or behind the sensor update that follows it): the state in (P, mean, var) into the slot the device words
// name.  The same arguments at every step of a buffer parity, so the launch may be captured.  No synchronisation.
int pnmol_record_enqueue(pnmol_filter* f, const double* P, const double* mean, const double* var);
// behind the call's synchronisation: the k slots take their times (t0 + dt, ...) and frame, the cursor moves
void pnmol_record_collect(pnmol_filter* f, double t0, int k, double dt);
// the cursor, and putting it back (pnmol_filter_prepare_steps rehearses a call)
int pnmol_record_cursor(const pnmol_filter* f);
void pnmol_record_rewind(pnmol_filter* f, int next);
void pnmol_record_free(pnmol_filter* f);

void pnmol_reaction_free_ws(pnmol_filter* f);
// pnmol_reaction.hip: enqueue k_linearize (k_linearize_system for a coupled system, k_linearize_convection for a convection
// term) on the ctx stream for one step over dt from the mean `mean` (Dp, in the frame frame_dt; 0 = raw coordinates): the
// diagonal (same-point; for a convection term all) slots of ell_val and the shift become those of the EK1 linearisation of the
// term at the predicted mean -- or, for a step of the loop (loop_step) while a table of linearisation points is set, at the row
// the device words name (the cursor word of the running call plus the loop's step counter; outside the loop those words name
// nothing, so pnmol_filter_linearize passes false).  Needs has_term(f); no synchronisation.  -2: the launch failed.
int pnmol_reaction_enqueue(pnmol_filter* f, const double* mean, double frame_dt, double dt, bool loop_step);
// pnmol_forcing.hip: the forcing inside pnmol_filter_step and pnmol_filter_steps_begin / _end.  table_set: a table of right-hand
// sides is set (the loop then runs non-fused: the next innovation cannot be prepared before its right-hand side is in place); set: a
// table, or a right-hand side of pnmol_filter_force_at (the operator setters then refuse).
bool pnmol_forcing_table_set(const pnmol_filter* f);
bool pnmol_forcing_set(const pnmol_filter* f);
// k_force in front of a step of the loop (the row the device words name) / of pnmol_filter_step (the row of pnmol_filter_force_at), on
// the ctx stream, behind the step's linearise launch if there is one.  Returns the shift the step measures with, NULL without a
// table / a right-hand side (nothing is enqueued then: the step reads f->shift as ever).  *rc = -2: the launch failed.
const double* pnmol_forcing_enqueue_loop(pnmol_filter* f, int* rc);
const double* pnmol_forcing_enqueue_single(pnmol_filter* f, int* rc);
void pnmol_forcing_free(pnmol_filter* f);
// pnmol_operator.hip: the time-dependent operator.  family_set: the operator setters and the wide terms refuse; schedule_set: a table
// of coefficients is set (the loop then runs non-fused: the next step's H is not in place before its row has been applied).
bool pnmol_operator_family_set(const pnmol_filter* f);
bool pnmol_operator_schedule_set(const pnmol_filter* f);
// with a family set: the values and the diagonal-slot table a pointwise reaction linearises on (the current operator and the union
// image's slots) in place of the creation-time ones; without: both pointers stay what they are
void pnmol_operator_linearize_base(const pnmol_filter* f, const double** base_val, const int** slot);
// the family's image with the current operator into ell_col / ell_val (grown if it is wider), and a zero shift: what
// pnmol_ell_restore_base is to a filter without a family.  Needs a family; the caller has dropped the graphs.
int pnmol_operator_put_image(pnmol_filter* f);
// k_operator_at in front of a step of the loop (the row the device words name), on the ctx stream, in front of the step's linearise
// launch.  Without a schedule nothing is enqueued.  -2: the launch failed.
int pnmol_operator_enqueue_loop(pnmol_filter* f);
void pnmol_operator_free(pnmol_filter* f);
// pnmol_loop_table.hip: the per-step tables (pnmol_filter::loop_tables).  A setter has validated and padded its rows and synchronised
// the stream; install uploads `count` rows of `stride` doubles: a table that fits the one before it is overwritten in place, one
// that does not is allocated first and swapped in only if that succeeded, a failed copy leaves no table set, and the captured
// graphs go or stay as loop_table_change says.  -4: out of memory, -2: another failure, ctx->err = who + the HIP error.  clear
// frees a table (its graphs go with it); free clears them all (pnmol_filter_destroy).
int loop_table_install(pnmol_filter* f, LoopTable* tab, const char* who, int count, int stride, const double* padded_rows);
void loop_table_clear(pnmol_filter* f, LoopTable* tab);
void loop_tables_free(pnmol_filter* f);
// what the pnmol_filter_*_pending functions report of a table
int loop_table_pending(const LoopTable& tab, int* next, int* count);
// the tables inside pnmol_filter_steps_begin / _end, as the recorder's functions above: the first refusal of a call of k steps in
// list order (-1, ctx->err set; nothing of HIP is touched), the cursor words of the running call on the ctx stream (once per call,
// in front of its steps), behind the call's synchronisation the cursors move (ok) or stay (the call failed), and the cursors and
// putting them back for a rehearsal.
int loop_tables_begin(pnmol_filter* f, int k);
int loop_tables_enqueue_cursors(pnmol_filter* f);
void loop_tables_collect(pnmol_filter* f, int k, bool ok);
struct LoopCursors {
    int next[LOOP_TABLES];
};
LoopCursors loop_tables_cursors(const pnmol_filter* f);
void loop_tables_rewind(pnmol_filter* f, const LoopCursors& c);
// pnmol_hip.hip: destroy the captured graphs of the constant-step loop
void pnmol_drop_graphs(pnmol_filter* f);
// pnmol_hip.hip: make ell_col / ell_val at least w slots wide.  Growing frees them (ellw = 0 until the caller has filled them): the
// caller has dropped the graphs and knows the stream idle.
int pnmol_ell_reserve(pnmol_filter* f, int w);
// pnmol_hip.hip: the image of the operator given at creation back into ell_col / ell_val, on the ctx stream.  For a term setter
// (for_term) the values are copied even over the base columns (k_linearize patches diagonal slots in place) and the shift is zeroed;
// pnmol_filter_set_operator_diagonal writes diagonal slots and shift itself, so nothing happens while ell_is_base, and a change of
// width drops the captured graphs.
int pnmol_ell_restore_base(pnmol_filter* f, bool for_term);

// The RTS smoother step (pnmol_smoother_step; pnmol_smooth.hip).
constexpr int SM_MAXN = 4;
struct SmoothConsts {
    double A1[SM_MAXN * SM_MAXN];  // IWP transition in the Nordsieck frame (IwpConsts.A1)
    double Q1[SM_MAXN * SM_MAXN];  // IwpConsts.Q1
    double ts[SM_MAXN];            // frame change of the filtered state into the frame of h
    double tsn[SM_MAXN];           // frame change of the smoothed successor into the frame of h
};

// Joint posterior draws (pnmol_samples_*; pnmol_sample.hip).  A sample block is
// Dp x Sp row-major (row = state component, derivative-major like a mean; column = draw, Sp = S rounded up to 64), the
// noise block 2 Dp x Sp (xi_1 over xi_2), padding zero.
struct SampleConsts {
    double A1[SM_MAXN * SM_MAXN];  // IwpConsts.A1
    double Q1[SM_MAXN * SM_MAXN];  // IwpConsts.Q1
    double Lq[SM_MAXN * SM_MAXN];  // chol(Q1), lower
    double ts[SM_MAXN];            // frame change of the filtered state into the frame of h
    double tsn[SM_MAXN];           // frame change of the sample block into the frame of h
};

// Dense output between grid times (pnmol_bridge_*, pnmol_state_predict*; pnmol_dense.hip).
// Point-diagonal block of an interval, the storage of a pnmol_bridge: [Pl | Cx | Pr] (each N*N rows of dp: entry (a, b) of the
// n x n block of the matrix at equal mesh points), [ml | mr] (N rows of dp each), diag K (dp).
inline size_t pnmol_dense_block_doubles(int n, int dp) { return (size_t)(3 * n * n + 2 * n + 1) * dp; }
struct DenseFrames {
    double sl[SM_MAXN];  // frame change applied to the left operand (mean: sl[a], covariance: sl[a] sl[b])
    double sr[SM_MAXN];  // the same for the right operand
};
// one row of the evaluation table: x_t = Bm x_l + Bp x_r + N(0, Qb (x) K), read out in raw coordinates through sc
struct DenseQuery {
    double Bm[SM_MAXN * SM_MAXN];
    double Bp[SM_MAXN * SM_MAXN];
    double qbd[SM_MAXN];  // diag Qb
    double sc[SM_MAXN];   // raw-coordinate scale of derivative a
    int knot;             // 0: the formula; 1 / 2: the stored values of the left / right end point
    int pad;
};
// the n x n matrices of the full-covariance kernel: BmS = Bm diag(sl), BpS = Bp diag(sr) carry the frame changes of Pl and Pr
struct DenseMix {
    double BmS[SM_MAXN * SM_MAXN], BpS[SM_MAXN * SM_MAXN], Bm[SM_MAXN * SM_MAXN], Bp[SM_MAXN * SM_MAXN], Qb[SM_MAXN * SM_MAXN];
};
// pnmol/base/iwp.py, bridge_coefficients, at the fraction th of a step: n x n matrices of row pitch MAXN
void bridge_coefficients(const pnmol_filter* f, double th, double* Bm, double* Bp, double* Qb);
// What a query inside [t_k, t_k + dt] needs, copied out of a smoother step's own buffers right behind it (tsn: the frame
// change of smooth_next).  On failure nothing is left behind and *bridge is NULL.
int pnmol_dense_make_bridge(pnmol_filter* f, const pnmol_state* filt_k, const pnmol_state* smooth_next, double dt,
                            const pnmol_state* out, const double* tsn, int keep_full, pnmol_bridge** bridge);
// The draw at t between (or behind) drawn neighbours: out = BmS xl [+ BpS xr] + Ls W on (Dp x Sp) sample blocks, the n x n mixes
// of the derivative blocks element-wise over points and draws (W = Gamma xi per derivative block; Ls lower triangular, scaled)
struct DenseDrawMix {
    double BmS[SM_MAXN * SM_MAXN], BpS[SM_MAXN * SM_MAXN], Ls[SM_MAXN * SM_MAXN];
};
int pnmol_dense_launch_draw_mix(hipStream_t st, int n, const DenseDrawMix& c, int dp, int Sp, const double* xl, const double* xr,
                                const double* W, double* out);
