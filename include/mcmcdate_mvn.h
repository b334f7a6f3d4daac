/*
 * mcmcdate_mvn.h -- C ABI of the MI355X-native MVN phylogenetic log-likelihood.
 *
 * Drop-in boundary for the ONE hot path of dschrempf/mcmc-date: the likelihood closure that the
 * `mcmc` sampler calls once per proposal.  Every entry point names the reference interface it
 * replaces (paths relative to the reference repository).  Plain pointers and sizes only; no
 * C++/torch types.  The library is libmcmcdate_mvn.so (built from mcmc-date_amd/csrc/ by
 * __graft_entry__.build()).  INTEGRATION.md shows the Haskell `foreign import ccall` stubs.
 *
 * Conventions
 *   - All arithmetic is IEEE fp64.  Log-likelihoods are log-domain values (the argument of
 *     `Exp` in Numeric.Log), exactly what app/Probability.hs:169 computes.
 *   - Return value: MCD_OK (0) or a negative MCD_ERR_* for STRUCTURAL faults (bad sizes, non-SPD
 *     matrix, non-bifurcating root, HIP failure) -- the reference raises `error` for these
 *     (app/Tools.hs:43, app/Main.hs:220,231).  NUMERIC faults are not errors: NaN/Inf inputs
 *     flow through to NaN / -Inf outputs so that Metropolis-Hastings rejects the proposal, as
 *     in the reference (lib/Mcmc/Tree/Proposal/Unconstrained.hs:304-306).
 *   - mcd_last_error() returns a thread-local message for the last failing call of this thread.
 *   - Handles are immutable after creation; every evaluation entry point is re-entrant and may
 *     be called concurrently from several OS threads on the same handle (the reference runs the
 *     closure from several threads under `-threaded -N`, mcmc-date.cabal:42, app/Main.hs:452).
 *   - Batches are CHAIN-MAJOR: chain b's vector is contiguous at base + b * ld (ld >= length).
 *   - `on_device` = 0: all data pointers are host pointers; the call copies, runs and returns
 *     synchronously.  `on_device` = 1: all data pointers are device pointers on the handle's
 *     GPU, the kernels are enqueued on `stream` (a hipStream_t passed as void*, NULL = default
 *     stream) and the call returns without synchronising.
 *   - Trees are described by a PRE-ORDER parent array (root = 0, parent[0] = -1, every node
 *     before its children, children left to right): the order of elynx-tree's `branches` and of
 *     the reference's Foldable instances (lib/Mcmc/Tree/Types.hs:91-95, 146-150).
 */
#ifndef MCMCDATE_MVN_H
#define MCMCDATE_MVN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCD_OK 0
#define MCD_ERR_INVALID_ARG (-1)
#define MCD_ERR_NOT_SPD (-2)              /* app/Main.hs:220, 231: prepare aborts on such a matrix  */
#define MCD_ERR_HIP (-3)
#define MCD_ERR_ROOT_NOT_BIFURCATING (-4) /* app/Tools.hs:43 "getBranches: Root node is not bifurcating." */
#define MCD_ERR_NO_DEVICE (-5)
#define MCD_ERR_UNSUPPORTED (-6)

#define MCD_MAT_SIGMA 0     /* `mat` is the covariance matrix Sigma (output of meanCov, app/Main.hs:208) */
#define MCD_MAT_SIGMA_INV 1 /* `mat` is Sigma^-1 as stored in <name>.data (FullS, app/Main.hs:81, 240)    */

#define MCD_MAX_DIM 1024    /* largest MVN dimension this build holds in registers */

typedef struct mcd_mvn mcd_mvn_t;   /* replaces the closure `likelihoodFunction (Full mu s d)`  */
typedef struct mcd_tree mcd_tree_t; /* topology tables for the state -> distances wrapper        */

/* Number of usable GPUs (0 when there is none; never fails). */
int mcd_device_count(void);
const char* mcd_version(void);
const char* mcd_last_error(void);

/*
 * Which form of the log-density kernels a launch uses (results agree to rounding, not bit for bit):
 *   MCD_FORM_AUTO     (default) by dimension and batch size: the column sweep up to N = 256 at a sampler's usual batch; for
 *                     N > 256 and up to 1024 chains (240 < N <= 256: up to 128) a row-split variant of the multiply form
 *                     (k_split.hip: the row blocks of L^-1 dealt to 8-32 workgroups per 16-chain tile, partial sums handed over
 *                     through a per-stream scratch owned by the handle), raw x and tree states alike; the multiply form from
 *                     2048 chains at N >= 96, from 8192 at N >= 32;
 *   MCD_FORM_SWEEP    always the column sweep (one chain per wave -- the latency form);
 *   MCD_FORM_MULTIPLY always the multiply form z = L^-1 (x - mu) on the fp64 matrix cores (the throughput form).
 * mcd_mvn_set_form chooses per handle (two samplers with a handle each can pin different forms); a handle whose choice is
 * MCD_FORM_AUTO follows the process default, which mcd_set_logpdf_form sets (a test and tuning knob; the environment
 * variable MCD_WIDE=0|1, read when the library is loaded, sets its initial value to SWEEP | MULTIPLY).  Both return the previous value.
 * The gradient entry points follow the same choice; above N = 256 the multiply form uses the gradient rows (`G`, `g_heights`)
 * as scratch while it runs: a call whose gradient array IS an input array (in place) takes the sweeps instead; partially
 * overlapping arrays are not supported by either form.  Above N = 768 the gradients have no sweep form (sixteen row blocks of both
 * sweeps' staging do not fit the register file): whatever the batch and the form asked for they take the row-split form in pieces
 * of at most 1024 chains; mcd_mvn_grad_batch may still be called in place, mcd_tree_grad_batch may write g_heights over heights and
 * g_rates over rates, but an output over the OTHER input array is refused there (MCD_ERR_HIP / invalid value).
 * Stream capture: every entry point that takes a stream may be captured into a hipGraph.  The row-split form gives a stream
 * under capture a scratch set of the capture's own, so a graph may be replayed on any stream while eager calls go on on the
 * stream it was captured from; two executable graphs instantiated from ONE capture must not be replayed concurrently.
 * A scratch set (256 KiB; gradient calls add two arrays of 1024 chains x 16 ceil(N/16) doubles, allocated at the first gradient
 * call) stays with its stream until the handle is destroyed.  A host that makes short-lived streams calls
 * mcd_mvn_release_stream(h, stream) before destroying one: it waits for the stream and returns its set to the handle's pool
 * (sets of captures stay with the capture: its graph may still be replayed).  hipStreamPerThread is keyed per calling thread.
 */
/*
 * Test and tuning knobs -- ONE explicit, thread-safe table instead of environment variables read on the hot path (rounds 1-3 called
 * getenv() per launch: a stray variable silently changed the launch structure and the rounding of a run, and getenv() races with setenv()
 * in a threaded host such as the reference's, mcmc-date.cabal:42-43).  name = "MCD_MH_SEGMENTS", "MCD_MH_INCREMENTAL", "MCD_MH_PER_PHASE",
 * "MCD_MH_PRIOR", "MCD_MH_PRIOR_CACHE", "MCD_MH_STEP_WG", "MCD_MH_CHAIN_LW", "MCD_MH_INC_SLOTS", "MCD_MH_SPARSE_SLOTS", "MCD_SPLIT", "MCD_SPLIT_G",
 * "MCD_SPLIT_SCATTER", "MCD_SPLIT_NOROT", "MCD_SPLIT_PROBE", "MCD_GEOM", "MCD_WIDE_CT", "MCD_SPARSE_QUAD", "MCD_MH_PRIOR_WAVES", "MCD_LOADERS",
 * "MCD_MH_SEG_TAIL" (0: a dense proposal after a segment is proposed by the step kernel), "MCD_MH_AHEAD_FROM" (nodes from which a segment's chain
 * wave draws the next proposal ahead of the decision), "MCD_MH_PRIOR_DRAWS" (0: no prior wave draws the next proposal's rejected branch),
 * "MCD_FSTREAM" (the column sweep's forward factor stream at 129 .. 256 dimensions: 0 = padded, 1 = compact, 2 = compact by LDS-DMA,
 * 3 = the inverse stream -- W = L^-1 in the compact layout, z = W (x - mu) without the substitution's dependent chain; it exists for
 * mcd_mvn_logpdf_batch at up to 512 chains, where 3 selects it under any form, and is the default there for 240 < N <= 256 at 129 .. 512
 * chains under form auto; elsewhere 3 means the default),
 * "MCD_SPARSE_GRAD_CHAINS" (1 | 2: chains per workgroup of mcd_sparse_tree_grad_batch; the same bits), "MCD_STRIPE_PROLOGUE" (the inverse
 * stream's kernel: 1 = x, mu and 1/diag loaded once per workgroup, 0 = by every wave for itself; the same bits), "MCD_STRIPE_SCHED" (that
 * kernel's schedule under the shared prologue: 1 = the column broadcasts read out of LDS and the ring read one group ahead of the
 * multiply-adds, 2 (the default) = that with the off-diagonal units loaded straight into registers where the sweep does not stop
 * early, 0 = the schedule before; the same bits), "MCD_STRIPE_FINISH" (where schedule 2 runs: 1 (the default) = each of a workgroup's two
 * chains is finished by a wave of its own, 0 = one wave finishes both; no effect elsewhere; the same bits), "MCD_STRIPE_DIAG" (where that finish runs: 1 = the diagonal parts of the
 * stream by register load like every other unit, no LDS ring, 0 = through the ring; unset = 1 for batches of 385 chains and more, where it is the faster one, else 0; no effect elsewhere;
 * the same bits);
 * value = a decimal integer, NULL or ""
 * = back to the default.  What each knob does is said where it acts (mcd_mh_run, the forms above).  The environment variables of the same
 * names are read ONCE, when the library is loaded, as initial values -- never afterwards.  No knob changes a result beyond rounding.
 */
int mcd_set_option(const char* name, const char* value);
int mcd_get_option(const char* name, int* is_set, int* value);

#define MCD_FORM_AUTO 0
#define MCD_FORM_SWEEP 1
#define MCD_FORM_MULTIPLY 2
int mcd_set_logpdf_form(int form);
int mcd_mvn_set_form(const mcd_mvn_t* h, int form);
int mcd_mvn_release_stream(const mcd_mvn_t* h, void* stream /* hipStream_t */);

/*
 * Build the immutable likelihood operands on GPU `device_id`.
 * Replaces: getLikelihoodFunction / getData (app/Main.hs:333-347, 85-99) + the closure creation
 * likelihoodFunction (Full mu sigmaInv logDetSigma) (app/Probability.hs:277-278, 247-248).
 *   n            MVN dimension (number of branches after merging the two root branches)
 *   mu           [n] posterior mean branch lengths
 *   mat          [n*n] row-major Sigma or Sigma^-1 (see mat_kind); only its symmetric part is used
 *   logdet_sigma log det Sigma; used as given when mat_kind = MCD_MAT_SIGMA_INV (the .data file
 *                carries it, app/Main.hs:240); ignored for MCD_MAT_SIGMA (computed from the factor)
 * The factors are computed on the host and staged on the device once: from Sigma its Cholesky factor; from Sigma^-1 = P the
 * factor W with P = W^T W directly (a reverse Cholesky factorisation: nothing is inverted twice) and L = W^-1 for the sweeps.
 * Contract, stricter than the reference's: the matrix must be numerically positive definite -- MCD_ERR_NOT_SPD otherwise.  (The
 * reference evaluates dx^T P dx with whatever P the .data file holds; `prepare` itself refuses a covariance matrix whose
 * determinant is not positive, app/Main.hs:231, so an indefinite P only arises from a hand-made file.  For such a matrix use the
 * product form, mcd_sparse_create below, which takes P as given -- the host mirrors' likelihoodFunction do so by themselves.)
 */
int mcd_mvn_create(mcd_mvn_t** out, int n, const double* mu, const double* mat, int mat_kind,
                   double logdet_sigma, int device_id);
void mcd_mvn_destroy(mcd_mvn_t* h);
int mcd_mvn_dim(const mcd_mvn_t* h);
int mcd_mvn_device(const mcd_mvn_t* h);
double mcd_mvn_logdet(const mcd_mvn_t* h);
/* Copy the row-major lower Cholesky factor [n*n] of Sigma to host memory (diagnostics/tests). */
int mcd_mvn_get_factor(const mcd_mvn_t* h, double* L_out);

/*
 * One evaluation, host pointers.  Exact drop-in for
 *   logDensityFullMultivariateNormal mu (sigmaInvH, logDetSigma) xs      (app/Probability.hs:166-173)
 * x: [n]; *ll receives c - 1/2 (logdet + (x-mu)^T Sigma^-1 (x-mu)).
 */
int mcd_mvn_logpdf(const mcd_mvn_t* h, const double* x, double* ll);

/* `batch` independent evaluations of the same function (one per chain).  X: chain-major, ld >= n. */
int mcd_mvn_logpdf_batch(const mcd_mvn_t* h, const double* X, int64_t ld, int64_t batch, int on_device,
                         void* stream, double* ll);

/*
 * Log-likelihood and its gradient with respect to x:  G[b] = -Sigma^-1 (x_b - mu).
 * Replaces the AD of logDensityMultivariateNormalG / reduceVMV (app/Probability.hs:286-326)
 * that mcmc's NUTS performs per leapfrog step (app/Hamiltonian.hs:86-92).  G: chain-major, ldg >= n.
 */
int mcd_mvn_grad_batch(const mcd_mvn_t* h, const double* X, int64_t ld, int64_t batch, int on_device,
                       void* stream, double* ll, double* G, int64_t ldg);

/*
 * Bind a tree topology to a likelihood (n_nodes = n + 2; bifurcating root required).
 * Replaces the traversal structure implicit in getBranches / sumFirstTwo (app/Tools.hs:36-48)
 * and heightTreeToLengthTree (lib/Mcmc/Tree/Types.hs:224-233).
 */
int mcd_tree_create(mcd_tree_t** out, const mcd_mvn_t* h, int n_nodes, const int32_t* parent);
void mcd_tree_destroy(mcd_tree_t* t);
int mcd_tree_n_nodes(const mcd_tree_t* t);

/*
 * State -> log-likelihood, the closure the sampler holds:
 *   likelihoodFunctionWrapper logDensityFullMultivariateNormal mu (sigmaInv, logdet) x
 *                                                                    (app/Probability.hs:195-207)
 * Per chain b:  heights[b*ld_state + v] = relative node heights of x^.timeTree (leaves 0, root 1),
 *               rates[b*ld_state + v]   = branch labels of x^.rateTree (index 0 = stem, unused),
 *               tH[b] = x^.timeHeight,  rMu[b] = x^.rateMean          (app/State.hs:70-89).
 * log_jac (may be NULL) receives jacobianRootBranch x = log (1 / rootBranch x)
 *                                                                    (app/Probability.hs:393-410).
 */
int mcd_tree_loglik_batch(const mcd_tree_t* t, const double* heights, const double* rates, int64_t ld_state,
                          const double* tH, const double* rMu, int64_t batch, int on_device, void* stream,
                          double* ll, double* log_jac);

/*
 * Log-likelihood and its gradient with respect to the state, replacing the AD of
 * likelihoodFunctionG (app/Probability.hs:361-388) in htargetWith (app/Hamiltonian.hs:72-92).
 * g_heights / g_rates: [batch][ld_state] (every node; masking per app/Hamiltonian.hs:33-47 is the
 * caller's business; g_rates[.][0] = 0), g_tH / g_rMu: [batch].  A chain whose ln likelihood is
 * NaN has NaN in every gradient entry (g_rates[.][0] included); no other chain is touched.
 */
int mcd_tree_grad_batch(const mcd_tree_t* t, const double* heights, const double* rates, int64_t ld_state,
                        const double* tH, const double* rMu, int64_t batch, int on_device, void* stream,
                        double* ll, double* g_heights, double* g_rates, double* g_tH, double* g_rMu);

/* ------------------------------------------------------------------------------------------------
 * Prior (built after the likelihood rows): the batched log prior of the state.
 * Replaces  priorFunction ht md cb cs bs :: PriorFunction I  (app/Probability.hs:127-150), i.e.
 *   calibrateConstrainBraceSoft (lib/Mcmc/Tree/Prior/Node/Combined.hs:70-92)
 *   * exponential 1 birth * exponential 1 death * birthDeath ConditionOnTimeOfMrca birth death 1 t'
 *                                                                  (lib/Mcmc/Tree/Prior/BirthDeath.hs:158-239)
 *   * exponential ht rMu * gamma (3/2) (1/6) rVar * relaxed clock model 1 rVar t' rateTree
 *                                                                  (lib/Mcmc/Tree/Prior/Branch/RelaxedClock.hs)
 * Node indices are pre-order ids (the reference's `identify`, Calibration.hs:173).  Calibration boundaries are
 * absolute ages; cal_has_lo/hi = 0 encodes `Zero` / `Infinity`.  Braces: CSR (brace_ptr[n_brace+1], brace_nodes).
 * State-dependent faults for which the reference calls `error` (variance <= 0, negative birth/death rate)
 * come back as NaN for that chain; probability 0 is -Inf.
 * ---------------------------------------------------------------------------------------------- */
#define MCD_CLOCK_UNCORRELATED_GAMMA 0
#define MCD_CLOCK_UNCORRELATED_LOGNORMAL 1
#define MCD_CLOCK_UNCORRELATED_WHITE_NOISE 2
#define MCD_CLOCK_AUTOCORRELATED_LOGNORMAL 3

typedef struct mcd_prior mcd_prior_t;

int mcd_prior_create(mcd_prior_t** out, int n_nodes, const int32_t* parent, double ht, int clock_model,
                     int n_cal, const int32_t* cal_node, const int32_t* cal_has_lo, const double* cal_lo,
                     const double* cal_lo_p, const int32_t* cal_has_hi, const double* cal_hi, const double* cal_hi_p,
                     int n_con, const int32_t* con_young, const int32_t* con_old, const double* con_p,
                     int n_brace, const int32_t* brace_ptr, const int32_t* brace_nodes, const double* brace_sd,
                     int device_id);
void mcd_prior_destroy(mcd_prior_t* p);

/* Per chain b: birth[b], death[b], tH[b], heights[b*ld_state + v], rMu[b], rVar[b], rates[b*ld_state + v]
 * (the seven fields of `I`, app/State.hs:70-89).  lp[b] = log prior; components (may be NULL): [b][3] =
 * node priors, birth-death block, relaxed-clock block (what app/Monitor.hs:27-57 monitors). */
int mcd_prior_logprior_batch(const mcd_prior_t* p, const double* birth, const double* death, const double* tH,
                             const double* heights, const double* rMu, const double* rVar, const double* rates,
                             int64_t ld_state, int64_t batch, int on_device, void* stream, double* lp,
                             double* components);

/*
 * Log prior and its gradient with respect to the seven fields of the state (first part): the prior
 * factor of the Hamiltonian target `htargetWith` (app/Hamiltonian.hs:72-92), which the reference differentiates by AD.
 * g_heights / g_rates: [batch][ld_state] (every node; masking per app/Hamiltonian.hs:33-47 is the caller's business;
 * g_rates[.][0] = 0).  Outside the support (ln prior = -inf or NaN) every gradient entry of that chain is NaN.  In the
 * near-critical regime of the birth-death prior (|birth - death| < 1e-6, BirthDeath.hs:117-118) the gradient is the one
 * of the exact formulas at the edge of that regime (relative deviation O(1e-6) from the first-order value's derivative).
 * Trees of up to 2048 nodes (MCD_ERR_UNSUPPORTED beyond: the kernel keeps 7 n_nodes + 2 doubles in LDS).
 */
int mcd_prior_grad_batch(const mcd_prior_t* p, const double* birth, const double* death, const double* tH,
                         const double* heights, const double* rMu, const double* rVar, const double* rates,
                         int64_t ld_state, int64_t batch, int on_device, void* stream, double* lp, double* g_birth,
                         double* g_death, double* g_tH, double* g_heights, double* g_rMu, double* g_rVar, double* g_rates);

/*
 * Leapfrog integrator of the Hamiltonian proposal on the device (second part).  Potential
 * U(q) = -ln [prior x likelihood x jacobianRootBranch] (`htargetWith`, app/Hamiltonian.hs:72-92); the position q is the
 * masked, reversed fold of the state (`getMask`, `toVector`, :33-53): root height, leaf heights and the rate stem are
 * fixed, the time height moves only when calibrations are available.  The state of `batch` chains lives on the device;
 *   mcd_hmc_set_state      host state in, evaluates ln target and its gradient
 *   mcd_hmc_get_position   q [batch][dim], ln target [batch], gradient [batch][dim] of the current state (any may be NULL)
 *   mcd_hmc_leapfrog       n_steps leapfrog steps with per-chain step size eps[b], per-chain direction dir[b] = +-1 (NULL
 *                          = forward) and diagonal inverse masses inv_mass[dim]; p [batch][dim] in/out (host)
 * A state that leaves the support gets NaN gradients; its momentum and ln target turn NaN (the caller rejects).
 *
 * The proposal itself -- `nuts` of the package `mcmc` (`nutsWith`, app/Hamiltonian.hs:95-105; not vendored), restated from the
 * algorithm it implements, Hoffman & Gelman (2014), Algorithm 3 -- runs on the device for all chains in lock step (k_nuts.hip:
 * slice variable, doubling in a random direction, U-turn and divergence stops, uniform choice among the admissible leaves;
 * in the default form of a transition, MCD_HMC_TRANSITION_ROUNDS, one round = the two gradient launches + one launch that finishes
 * the leapfrog step, books the leaf and sends the next one on its way, and the host only polls a counter; a handle over a small
 * tree may take the whole transition as one launch instead: mcd_hmc_set_transition_form below):
 *   mcd_hmc_nuts        one transition from the handle's state with per-chain step sizes eps[batch] and inverse masses
 *                       inv_mass[dim]; random streams: Philox (seed, chain_offset + b, transition) -- a chain's draw does not
 *                       depend on the batch it runs in; out: mean acceptance statistic alpha[batch], tree depth[batch].
 *                       The streams share the counter layout of mcd_mh_*: a host that runs both on one seed passes
 *                       seed ^ constant here (the Python mirror: hmc.NUTS_STREAM_DOMAIN) and a transition counter that never
 *                       restarts.  After the call the handle holds the accepted point with its value and gradient, so any
 *                       entry point (mcd_hmc_leapfrog, mcd_hmc_get_position, another transition) may follow directly.
 *   mcd_hmc_nuts_run    n transitions; adapt != 0: dual averaging of the step sizes towards the acceptance statistic delta
 *                       (Algorithm 6; eps in: starting value, out: the averaged value); mean_alpha[batch]; q_mean / q_var[dim]:
 *                       position means and variances pooled over chains and transitions (what a mass adaptation needs:
 *                       the reference tunes `HTuneLeapfrog HTuneAllMasses`, app/Hamiltonian.hs:62-63; the diagonal form of that
 *                       tuning is mcd_hmc_nuts_warmup, the full mass matrix mcd_hmc_set_metric / mcd_hmc_nuts_warmup_dense below).
 * `mcmc`'s own defaults and tuning schedule are not available here: parity of this part rests on the CPU twin
 * (tests/test_gpu_nuts.py) and on the agreement with Metropolis-Hastings chains.
 */
typedef struct mcd_hmc mcd_hmc_t;
int mcd_hmc_create(mcd_hmc_t** out, const mcd_tree_t* tree, const mcd_prior_t* prior, int calibrations_available, int64_t batch);
void mcd_hmc_destroy(mcd_hmc_t* m);
int mcd_hmc_dim(const mcd_hmc_t* m);
int mcd_hmc_set_state(mcd_hmc_t* m, const double* birth, const double* death, const double* tH, const double* heights,
                      const double* rMu, const double* rVar, const double* rates, int64_t ld_state);
int mcd_hmc_get_state(const mcd_hmc_t* m, double* birth, double* death, double* tH, double* heights, double* rMu,
                      double* rVar, double* rates, int64_t ld_state);
int mcd_hmc_get_position(const mcd_hmc_t* m, double* q, double* value, double* grad);
int mcd_hmc_leapfrog(mcd_hmc_t* m, double* p, const double* eps, const double* dir, const double* inv_mass, int n_steps);
int mcd_hmc_nuts(mcd_hmc_t* m, const double* eps, const double* inv_mass, int max_depth, uint64_t seed, int64_t chain_offset,
                 uint64_t transition, double* alpha, int32_t* depth);
int mcd_hmc_nuts_run(mcd_hmc_t* m, int n_transitions, int adapt, double* eps, const double* inv_mass, double delta, int max_depth,
                     uint64_t seed, int64_t chain_offset, uint64_t first_transition, double* mean_alpha, double* q_mean, double* q_var);
/* Step sizes AND masses (`HTuneLeapfrog HTuneAllMasses`, app/Hamiltonian.hs:62-63): `windows` windows of `window` transitions --
 * dual averaging of eps[batch] inside a window, then inv_mass[dim] := pooled variance of the positions the window visited
 * (shrunk towards 1e-3) -- and a closing window for the step sizes; uses the transitions first_transition ..
 * first_transition + (windows + 1) window - 1 of the random streams.  eps, inv_mass: in = starting values, out = tuned. */
int mcd_hmc_nuts_warmup(mcd_hmc_t* m, int windows, int window, double* eps, double* inv_mass, double delta, int max_depth, uint64_t seed,
                        int64_t chain_offset, uint64_t first_transition, double* mean_alpha);
/*
 * The FULL mass matrix (`HTuneAllMasses`): a dense metric set on the handle replaces the vector inv_mass of every entry point.
 * With C = M^-1 = U U^T (U the lower Cholesky factor, taken on the host or, by mcd_hmc_set_metric_factor, on the device): momenta p = U^-T z from the normal draws z of the diagonal
 * form (so cov p = C^-1 = M), kinetic energy 1/2 p^T C p, drift q += eps (C p), U-turn test (q+ - q-)^T C r >= 0 at both ends; slice,
 * doubling, reservoir, merge, divergence test and random streams are those of the diagonal form.  Every product v = C x is one
 * workgroup's sum over j ascending with one accumulator per coordinate: a chain's bits depend on nothing but the chain.
 *   mcd_hmc_set_metric   inv_mass_dense = C [dim][dim] row-major (host); NULL clears the dense metric, and the handle is again what it
 *                        was before.  Refused with MCD_ERR_INVALID_ARG, the handle untouched, the message naming the first offender:
 *                        a non-finite entry; |C_ij - C_ji| > 1e-10 sqrt(C_ii C_jj); not positive definite (the pivot).  Refused with
 *                        MCD_ERR_UNSUPPORTED: dim > MCD_HMC_DENSE_MAX_DIM in the default form (C is read once per product and chain
 *                        out of the L2; beyond, the right form is one multiply across the lock-step chains: mcd_hmc_set_metric_form),
 *                        dim > MCD_HMC_DENSE_ACROSS_MAX_DIM -- more than any handle has -- in the across-chains form.  The handle keeps
 *                        (C + C^T) / 2, exactly symmetric, and U^-1 on its device.
 *   mcd_hmc_set_metric_form   how the products with C and U^-1 are taken.  MCD_HMC_METRIC_PER_CHAIN (the default): one workgroup's sum
 *                        per chain, dim <= MCD_HMC_DENSE_MAX_DIM.  MCD_HMC_METRIC_ACROSS_CHAINS: the chains of a transition are in lock
 *                        step, so the products of a round are rows of ONE matrix product on the fp64 matrix cores (k_metric_gemm.hip);
 *                        every dim, the same definitions, draws and order of decisions; a chain's bits still depend on nothing but the
 *                        chain (the order of every sum is a function of dim alone), but they are not the per-chain form's bits.
 *                        Allowed only while no dense metric is set (else MCD_ERR_INVALID_ARG, the handle untouched; a value that is
 *                        neither form likewise); the form survives mcd_hmc_set_metric(NULL) and is followed by
 *                        mcd_hmc_nuts_warmup_dense.  mcd_hmc_get_metric_form: *form = the handle's form.
 *   mcd_hmc_set_metric_factor   where the factors are taken.  MCD_HMC_FACTOR_HOST (the default): the host's long double loops, then C and
 *                        U^-1 are uploaded.  MCD_HMC_FACTOR_DEVICE: mcd_hmc_set_metric keeps its checks of the host array and their
 *                        messages, uploads C once, and the symmetric part, U and U^-1 are taken on the device (k_metric_factor.hip: a
 *                        blocked factorisation on the fp64 matrix cores; the same definitions entry by entry, plain double sums in
 *                        another order, so the factors differ from the host's in the last bits and are the same bits on every call);
 *                        they become the handle's only when the device reports success, and a refusal names the pivot in the same
 *                        words.  mcd_hmc_nuts_warmup_dense then shrinks, symmetrises and factors every window's covariance where
 *                        k_hmc_cov.hip left it, and the host copy of C is fetched when mcd_hmc_get_metric or inv_mass_dense_out asks
 *                        for it.  A per-handle choice, allowed at any time (it decides the NEXT factorisation); it survives
 *                        mcd_hmc_set_metric(NULL); any other value is MCD_ERR_INVALID_ARG, the handle untouched.
 *                        mcd_hmc_get_metric_factor: *where = the handle's choice.
 *   mcd_hmc_get_metric   *is_dense = 0 / 1; inv_mass_dense (may be NULL) receives the stored symmetrised C when dense.
 * While a dense metric is set, mcd_hmc_leapfrog, mcd_hmc_step_from, mcd_hmc_nuts and mcd_hmc_nuts_run require inv_mass == NULL
 * (a vector is MCD_ERR_INVALID_ARG: no caller silently runs the other metric); with none set, NULL stays the error it was.
 *   mcd_hmc_nuts_warmup_dense   the schedule of mcd_hmc_nuts_warmup (windows >= 1, window >= 1) from the diagonal inv_mass0[dim] -- a
 *                        dense metric on the handle is cleared first --: after every window
 *                        C = n / (n + 5) Cov + 1e-3 5 / (n + 5) I, n = batch window, Cov the centred covariance (divided by n) of the
 *                        n positions the window visited, computed on the device in a fixed order (k_hmc_cov.hip); a window whose
 *                        covariance is not finite or has no Cholesky factor leaves the metric as it was.  A closing window adapts eps
 *                        to the final metric, which stays SET ON THE HANDLE and is copied to inv_mass_dense_out [dim][dim] (may be
 *                        NULL); eps: in = starting values, out = tuned.  Transitions first_transition .. first_transition +
 *                        (windows + 1) window - 1; the recorder's room is checked up front for all of them.
 */
#define MCD_HMC_DENSE_MAX_DIM 512
#define MCD_HMC_METRIC_PER_CHAIN 0
#define MCD_HMC_METRIC_ACROSS_CHAINS 1
#define MCD_HMC_DENSE_ACROSS_MAX_DIM 4098 /* 2 * 2048 + 2: every dim an mcd_hmc_t can have */
int mcd_hmc_set_metric(mcd_hmc_t* m, const double* inv_mass_dense);
int mcd_hmc_set_metric_form(mcd_hmc_t* m, int form);
int mcd_hmc_get_metric_form(const mcd_hmc_t* m, int* form);
int mcd_hmc_get_metric(const mcd_hmc_t* m, int* is_dense, double* inv_mass_dense);
int mcd_hmc_nuts_warmup_dense(mcd_hmc_t* m, int windows, int window, double* eps, const double* inv_mass0, double delta, int max_depth,
                              uint64_t seed, int64_t chain_offset, uint64_t first_transition, double* mean_alpha, double* inv_mass_dense_out);
#define MCD_HMC_FACTOR_HOST 0
#define MCD_HMC_FACTOR_DEVICE 1
int mcd_hmc_set_metric_factor(mcd_hmc_t* m, int where);
int mcd_hmc_get_metric_factor(const mcd_hmc_t* m, int* where);
/*
 * How a transition is launched, per handle.  MCD_HMC_TRANSITION_ROUNDS (the default): the rounds described above, three launches and one
 * host poll per leapfrog step of a tree.  MCD_HMC_TRANSITION_ONE_LAUNCH: a whole transition of every chain -- momenta, slice, every
 * doubling with its gradients, the U-turn and divergence stops, the choice of the proposal, the evaluation at the accepted point -- is
 * ONE kernel launch (k_nuts_chain.hip: a workgroup per chain, no host poll inside), and the n_steps leapfrog steps of mcd_hmc_leapfrog are
 * one launch.  It holds for mcd_hmc_nuts, mcd_hmc_nuts_run, mcd_hmc_nuts_warmup, mcd_hmc_nuts_warmup_dense, every transition of a handle
 * attached to a sampler (mcd_mh_attach_hamiltonian) and mcd_hmc_leapfrog; mcd_hmc_step_from and mcd_hmc_set_state run as they do, and the
 * recorder's store, the position moments, the covariance and the hand-over stay the launches they are, after the transition's.  The host
 * still waits once per transition where it does today.
 *   Eligible: a handle of mcd_hmc_create (dense likelihood) of at most 64 distances -- a tree of at most 66 nodes: one 64-row block of
 *   the factor, which one workgroup keeps in LDS -- with the diagonal metric or a dense one in MCD_HMC_METRIC_PER_CHAIN.  Refused with
 *   MCD_ERR_UNSUPPORTED, the handle untouched, the message naming the reason and both numbers: a handle of mcd_hmc_create_sparse, more
 *   than 64 distances, a handle in MCD_HMC_METRIC_ACROSS_CHAINS -- and mcd_hmc_set_metric_form(MCD_HMC_METRIC_ACROSS_CHAINS) on a
 *   one-launch handle likewise.  Any other value: MCD_ERR_INVALID_ARG.  The form may be set at any time between calls; it survives
 *   mcd_hmc_set_state, mcd_hmc_set_metric(NULL), mcd_hmc_take_state and mcd_hmc_record_begin / _end.
 *   The same bits: every output of those entry points -- state, position, ln target, gradient, alpha, depth, tuned step sizes, masses and
 *   metric, moments, recorder samples with their diagnostics, mcd_mh_hamiltonian_stats, and the gradient kernels' raw outputs, which
 *   belong to the accepted point afterwards -- is bit for bit what the rounds form gives WHEN ITS LIKELIHOOD GRADIENT RUNS THE
 *   SUBSTITUTION SWEEP, which is what the automatic choice takes at a sampler's batch.  From 2048 chains, or under a forced form
 *   (mcd_mvn_set_form, MCD_FORM), the rounds form's likelihood gradient is the multiply form, with that form's bits; the one-launch
 *   form does not follow it and keeps the sweep's.
 *   mcd_hmc_get_transition_form: *form = the handle's form.
 */
#define MCD_HMC_TRANSITION_ROUNDS 0      /* the default: what runs today */
#define MCD_HMC_TRANSITION_ONE_LAUNCH 1
int mcd_hmc_set_transition_form(mcd_hmc_t* m, int form);
int mcd_hmc_get_transition_form(const mcd_hmc_t* m, int* form);
/*
 * The factors of a dense metric without a handle, on host arrays: C [dim][dim] row-major; sym receives (C + C^T) / 2 with the diagonal of
 * C, U the lower triangular factor (U U^T = sym), Uinv = U^-1, both with +0.0 above the diagonal, [dim][dim] each; any of the three may be
 * NULL.  where = MCD_HMC_FACTOR_HOST: what mcd_hmc_set_metric computes by default, no device is touched.  MCD_HMC_FACTOR_DEVICE: the kernels
 * behind mcd_hmc_set_metric_factor on device_id; without a device MCD_ERR_NO_DEVICE (no fall-back to the host).  Refused as
 * mcd_hmc_set_metric refuses, with its messages (MCD_ERR_INVALID_ARG, the outputs untouched); dim > MCD_HMC_DENSE_ACROSS_MAX_DIM:
 * MCD_ERR_UNSUPPORTED.  info [3] (may be NULL): MCD_METRIC_FACTOR_* , then row and column of the offending entry (the pivot twice).
 */
#define MCD_METRIC_FACTOR_OK 0
#define MCD_METRIC_FACTOR_NOT_FINITE 1 /* C[row][col] is NaN or infinite                              */
#define MCD_METRIC_FACTOR_DIAGONAL 2   /* C[row][row] <= 0                                            */
#define MCD_METRIC_FACTOR_ASYMMETRIC 3 /* |C[row][col] - C[col][row]| > 1e-10 sqrt(C_rowrow C_colcol) */
#define MCD_METRIC_FACTOR_PIVOT 4      /* the Cholesky factorisation fails at pivot row                */
int mcd_metric_factor(int dim, const double* C, int where, int device_id, double* sym, double* U, double* Uinv, int64_t* info);
/*
 * The sample recorder of the NUTS driver: thinned samples of every chain AND the diagnostics of the transitions behind them kept ON THE
 * DEVICE while mcd_hmc_nuts / _nuts_run / _nuts_warmup run.  Replaces: the `monitor` of app/Definitions.hs:288-417 (`mcmc`'s MonitorFile
 * with period 2 everywhere) for runs with `--hamiltonian`, as the source of the states that the monitor files and scripts/analyze read --
 * without one mcd_hmc_nuts call and one mcd_hmc_get_state per transition -- and what `mcmc` prints of its NUTS proposal.  The contracts are
 * those of mcd_mh_record_* (below) point for point; the ring holds the same records, read by the same kernels.
 *   mcd_hmc_record_begin   a ring of capacity_samples slots on the handle's device; the transition count starts at 0.  period >= 1,
 *                          capacity_samples >= 1; one recorder per handle (a second begin without end is refused).
 *   mcd_hmc_nuts*          while a recorder is active every transition counts, through whichever of the three entry points, so calls of
 *                          any lengths give the samples of one long call; after every transition whose number is a multiple of period
 *                          the state of every chain is stored as one sample (k_hmc_record.hip).  A call whose samples do not fit the
 *                          free slots returns MCD_ERR_INVALID_ARG before anything is launched (the message names both numbers) and leaves
 *                          the handle as it was: _nuts_run and _nuts_warmup count their transitions up front, mcd_hmc_nuts is refused when
 *                          its transition would be sampled and the ring is full.  The chains do not change: end state, alpha, depth, the
 *                          tuned eps, the masses and q_mean / q_var are the same bits with and without a recorder.  On the device sample
 *                          number k goes to slot (k - 1) mod capacity, so no store can leave the ring.  If a call fails after it has
 *                          launched (MCD_ERR_HIP), the recorder's count no longer matches the chains: end the recorder.
 *   mcd_hmc_record_count   samples waiting to be fetched.
 *   mcd_hmc_record_fetch   waits for the handle's stream, copies the oldest *n_out = min(waiting, max_samples) samples to the host,
 *                          sample-major, and frees their slots: transition[n] (counted from begin), scalars[n][batch][5] (birth, death,
 *                          tH, rMu, rVar), heights / rates[n][batch][n_nodes], post[n][batch][3] (ln prior, ln likelihood, ln
 *                          jacobianRootBranch of the accepted state; their sum is mcd_hmc_get_position's value re-evaluated),
 *                          nuts[n][batch][6]: tree depth, leapfrog steps, acceptance statistic (the alpha of mcd_hmc_nuts), diverged (1: a
 *                          leaf failed the Delta_max test or left the support), the step size used, -H at the start of the transition.
 *                          Any of the arrays may be NULL.
 *   mcd_hmc_record_end     frees the ring.  mcd_hmc_set_state leaves an active recorder and its count alone; mcd_hmc_destroy frees it.
 *   mcd_hmc_record_quantities / mcd_hmc_record_summary   as mcd_mh_record_quantities / mcd_mh_record_summary (same quantities, same order,
 *                          same columns, same refusals before any launch, the same bits on every call, no slot freed); nuts_stats
 *                          [batch][4] (may be NULL): per chain over the window divergent transitions, mean tree depth, maximum tree
 *                          depth, leapfrog steps.
 * Dense and sparse handles alike.
 */
int mcd_hmc_record_begin(mcd_hmc_t* m, int32_t period, int64_t capacity_samples);
int mcd_hmc_record_count(const mcd_hmc_t* m, int64_t* n_samples);
int mcd_hmc_record_fetch(mcd_hmc_t* m, int64_t max_samples, int64_t* n_out, int64_t* transition, double* scalars, double* heights, double* rates,
                         double* post, double* nuts);
int mcd_hmc_record_end(mcd_hmc_t* m);
int mcd_hmc_record_quantities(const mcd_hmc_t* m, int64_t* q);
int mcd_hmc_record_summary(mcd_hmc_t* m, int64_t skip, int64_t n_samples, int32_t max_lag, int64_t* n_used, double* pooled, double* per_chain,
                           double* nuts_stats);
/* One leapfrog step from ARBITRARY phase points (what a NUTS tree needs: it extends either end of a trajectory):
 * q, p, grad [batch][dim] in/out (host), value [batch] out (ln target at the new point, may be NULL).  have_grad = 0:
 * the gradient at q is evaluated first (grad is output only).  The handle's own state becomes the new point. */
int mcd_hmc_step_from(mcd_hmc_t* m, double* q, double* p, double* grad, int have_grad, const double* eps, const double* dir,
                      const double* inv_mass, double* value);

/* ------------------------------------------------------------------------------------------------
 * Batched Metropolis-Hastings-Green driver (FIRST SLICE).  `mcmc`'s `mhg` evaluates one state
 * per call (app/Main.hs:474); here `batch` independent chains execute the same proposal of the cycle at the same
 * time, each with its own random numbers, tuning parameter and accept/reject decision.  The state never leaves
 * the device between calls.  A proposal is a row of the table below; the caller builds the table and the
 * per-iteration order (the reference: app/Definitions.hs:127-278 `proposals`, weights replicated and shuffled by
 * `mcmc`).  Every proposal of the reference cycle is a kind below; the Hamiltonian proposal of `--hamiltonian` (NUTS,
 * app/Hamiltonian.hs, row f3) is no kind of the table: it is an mcd_hmc_t attached to the driver (mcd_mh_attach_hamiltonian, below).
 * ---------------------------------------------------------------------------------------------- */
#define MCD_PROP_SCALE_SCALAR 0        /* scaleUnbiased k [mcmc]: node = 0 birth, 1 death, 2 tH, 3 rMu, 4 rVar; p0 = k          */
#define MCD_PROP_SLIDE_NODE 1          /* slideNodeAtUltrametric (Ultrametric.hs:50-59): node; p0 = sd                          */
#define MCD_PROP_SCALE_SUBTREE_TIME 2  /* scaleSubTreeAtUltrametric (:126-149): node; p0 = sd; n1 = inner nodes of the sub tree  */
#define MCD_PROP_PULLEY 3              /* pulleyUltrametric (:221-286): p0 = sd; n1, n2 = inner nodes left / right               */
#define MCD_PROP_SCALE_BRANCH_RATE 4   /* scaleBranch (Unconstrained.hs:40-66): node; p0 = shape                                 */
#define MCD_PROP_SCALE_SUBTREE_RATE 5  /* scaleTree on a sub tree (:84-130): node; p0 = shape; n1 = nodes of the sub tree        */
#define MCD_PROP_SCALE_NORM_TREE 6     /* scaleNormAndTreeContrarily (:221-256): node = 2 (tH) or 3 (rMu); p0 = shape            */
#define MCD_PROP_SCALE_VAR_TREE 7      /* scaleVarianceAndTree (:286-316): p0 = shape; p1 = 1 uses the determinant u^(n-1) as
                                          Jacobian instead of the reference's (u - u/n + 1/n)^n            */
#define MCD_PROP_SCALE_VAR_TREE_AUTO 8 /* scaleVarianceAndTreeAutocorrelated (:354-386): p0 = shape                              */
#define MCD_PROP_SCALE_CONTRARILY 9    /* scaleContrarily k th [mcmc] on (tH, rMu): p0 = k, p1 = th                              */
#define MCD_PROP_SLIDE_NODE_CONTRA 10  /* slideNodesAtContrarily (Contrary.hs:35-77): node; p0 = sd                              */
#define MCD_PROP_SCALE_SUBTREE_CONTRA 11 /* scaleSubTreesAtContrarily (:269-326): node; p0 = sd; n1 = inner nodes, n2 = nodes    */
#define MCD_PROP_SLIDE_ROOT_CONTRA 12  /* slideRootContrarily (:191-223) on (tH, time tree, rate tree): p0 = sd; n1 = exponent of
                                          1/u in the Jacobian: the reference passes the number of inner nodes INCLUDING the root */
#define MCD_PROP_SCALE_RATES_TREE_CONTRA 13 /* scaleRatesAndTreeContrarily (:420-446) on (birth rate, rate mean, time tree):
                                          p0 = sd; n1 = inner nodes - 1                                                         */
#define MCD_PROP_SLIDE_BRACE 14        /* slideBracedNodesUltrametric (Brace.hs:98-156): node = brace index of the prior; p0 = sd */
#define MCD_PROP_SLIDE_BRACE_CONTRA 15 /* slideBracedNodesContrarily (Brace.hs:37-61): node = brace index; p0 = sd                */

typedef struct mcd_mh mcd_mh_t;

/*
 * tree, prior: handles on the same device; they must outlive the driver.  Proposal table, n_prop rows: kind, node,
 * n1, n2 (see above), jac_root = 1 for proposals lifted with jacobianRootBranch (the "[R]" proposals of
 * app/Definitions.hs:145-278), dim = PDimension (selects the optimal acceptance rate of the auto tuner), p0, p1.
 * All chains start with tuning parameter 1.  Random numbers are Philox4x32-10 keyed by `seed`, counter =
 * (draw, chain, step): results do not depend on batch size, launch geometry or GPU count.
 * Unlike the likelihood and prior handles, a driver handle (mcd_mh_t, mcd_hmc_t) carries the chains' state: use it from
 * one thread at a time; different handles may be driven concurrently from different threads.
 */
int mcd_mh_create(mcd_mh_t** out, const mcd_tree_t* tree, const mcd_prior_t* prior, int n_prop, const int32_t* kind,
                  const int32_t* node, const int32_t* n1, const int32_t* n2, const int32_t* jac_root, const int32_t* dim,
                  const double* p0, const double* p1, int64_t batch, uint64_t seed);
/* The same driver over a likelihood whose precision matrix stays sparse on the device (mcd_sparse_tree_create): the reference's PRODUCTION
 * configuration -- `mhg` with likelihoodFunction (Sparse ...) (app/Main.hs:474, 257-277, 333-347; app/Probability.hs:178-184, 279); every
 * published timing of the reference uses it.  Trees of 3 .. 2048 nodes (a Sparse record never has to be densified).  mcd_mh_run takes the
 * segment structure (MCD_MH_PATH_SEGMENTS_SPARSE): every run of steps between two proposals that move more than 254 distances in ONE launch,
 * the chains' states in LDS, the quadratic form q = dx^T P dx kept per chain and updated through the ROWS of the moved distances,
 *     q' = q + sum_{j moved} delta_j sum_k Ps[j][k] (2 dx_k + delta_k),   Ps = (P + P^T) / 2;
 * such a dense proposal by two launches (the step kernel proposes, the one-launch full form evaluates), q recomputed by a full form every
 * 256 steps.  On a tree whose distances all fit the list (at most 256 nodes) every proposal runs inside a segment.  MCD_MH_SEGMENTS=0 or
 * MCD_MH_INCREMENTAL=0 (mcd_set_option): the step kernel + a full product at every step (round 3's structure; the chains: same decisions and
 * states).  Everything else (mcd_mh_set_state, _run, _tune, _mc3_*, ...) as for mcd_mh_create.  The mcd_sparse_tree_t type is declared with
 * the sparse form below. */
struct mcd_sparse_tree;
int mcd_mh_create_sparse(mcd_mh_t** out, const struct mcd_sparse_tree* tree, const mcd_prior_t* prior, int n_prop, const int32_t* kind,
                         const int32_t* node, const int32_t* n1, const int32_t* n2, const int32_t* jac_root, const int32_t* dim,
                         const double* p0, const double* p1, int64_t batch, uint64_t seed);
void mcd_mh_destroy(mcd_mh_t* m);
/* first_chain: global index of this handle's chain 0 (chain shards on several GPUs draw disjoint random streams). */
int mcd_mh_set_chain_offset(mcd_mh_t* m, int64_t first_chain);
/* Host arrays, the seven fields of `I` per chain (as mcd_prior_logprior_batch); evaluates the posterior. */
int mcd_mh_set_state(mcd_mh_t* m, const double* birth, const double* death, const double* tH, const double* heights,
                     const double* rMu, const double* rVar, const double* rates, int64_t ld_state);
int mcd_mh_get_state(const mcd_mh_t* m, double* birth, double* death, double* tH, double* heights, double* rMu,
                     double* rVar, double* rates, int64_t ld_state);
/* post: [batch][3] = ln prior, ln likelihood, ln jacobianRootBranch of the current states. */
int mcd_mh_get_posterior(const mcd_mh_t* m, double* post);
/*
 * n_iter iterations of steps_per_iter proposals; schedule[n_iter * steps_per_iter] = proposal row per step (host).
 * accumulate != 0: after every iteration add the absolute node ages tH * h_v to the running sums.
 * trace_alpha / trace_accept (host, may be NULL): [n_iter * steps_per_iter][batch] ln acceptance ratio / decision.
 * Which launch structure a run takes (mcd_mh_last_path) is decided once, when the run starts, from the handle's shape and the knobs below:
 * - trees of at most 64 nodes (dense likelihood): the whole schedule in one launch, the factor of Sigma in LDS (path 1, any batch);
 * - 65 .. 258 nodes (N <= 256) at up to 1024 chains, unless the multiply form is forced: the same with the factor streamed through LDS once
 *   per step (path 2);
 * - 259 .. 1026 nodes: every run of steps between two proposals that move more than 192 branch distances in one launch, the chains' states
 *   in LDS (k_mh_segment.hip); such a dense proposal by a likelihood launch (path 8, any batch);
 * - a sparse likelihood (mcd_mh_create_sparse), 3 .. 2048 nodes: the same segments over the rows of the matrix (path 9);
 * - otherwise two launches per step -- accept the pending proposal and propose the next one; then the ln likelihood of the proposed states:
 *   65 .. 258 nodes beyond 1024 chains, the likelihood launch carrying the proposal's ln prior as workgroups of a second role where the
 *   column sweep serves it (path 3; else path 4, e.g. from 2048 chains, where the multiply form takes over).
 * Knobs (mcd_set_option), for tests and timing; the chains are the same bits on every path:
 * MCD_MH_PER_PHASE=1 takes two launches per step instead of paths 1 and 2 (for path 1 it must be set before mcd_mh_create);
 * MCD_MH_SEGMENTS=0 switches the segments off: 259 .. 320 nodes then take path 4, from 321 nodes the workgroup-per-chain step kernel with the
 * likelihood launch only for proposals that move more than 32 distances (path 6), a sparse likelihood the step kernel + the sparse product
 * at every step (path 7); MCD_MH_INCREMENTAL=0 switches every incremental evaluation off as well: path 2 sweeps every proposal, from 321
 * nodes path 5 (a full product at every step), a sparse likelihood path 7;
 * MCD_MH_STEP_WG=1 / 0 forces / forbids the workgroup-per-chain step kernel (default: trees of more than 320 nodes, 258 with the segments;
 * the sparse driver refuses 0); MCD_MH_PRIOR=0 evaluates the prior inside the step kernel everywhere (path 4 instead of 3);
 * MCD_MH_CHAIN_LW=0 runs path 1 with one wave per chain (the likelihood after the prior instead of beside it);
 * MCD_MH_INC_SLOTS (read by mcd_mh_create) sets the number of moved distances up to which a proposal counts as sparse (at most 256),
 * MCD_MH_SPARSE_SLOTS the same for path 2 (at most 64).
 */
int mcd_mh_run(mcd_mh_t* m, const int32_t* schedule, int64_t n_iter, int32_t steps_per_iter, int accumulate,
               double* trace_alpha, int8_t* trace_accept);
/* Which launch structure the last mcd_mh_run took (reporting: bench.py, tests). */
#define MCD_MH_PATH_NONE 0
#define MCD_MH_PATH_CHAIN_LDS 1               /* whole schedule in one launch, factor resident in LDS (<= 64 nodes) */
#define MCD_MH_PATH_CHAIN_STREAMED 2          /* whole schedule in one launch, factor streamed once per step (k_mh_chain_big) */
#define MCD_MH_PATH_TWO_LAUNCH_PRIOR_BESIDE 3 /* step + likelihood launch that also carries the ln prior of the proposal */
#define MCD_MH_PATH_TWO_LAUNCH 4              /* step (prior inside) + likelihood launch */
#define MCD_MH_PATH_STEP_WG_X 5               /* workgroup-per-chain step leaving distances + plain-vector likelihood launch */
#define MCD_MH_PATH_STEP_WG_INCREMENTAL 6     /* the same, the likelihood launch only for proposals that move many distances (k_mh_inc.hip) */
#define MCD_MH_PATH_STEP_WG_SPARSE 7          /* workgroup-per-chain step leaving distances + the sparse product on them (mcd_mh_create_sparse) */
#define MCD_MH_PATH_SEGMENTS 8                /* 259 .. 1026 nodes: every run of steps between two dense proposals in one launch (state in LDS); a dense proposal: proposed by the segment before it (else by path 6's step kernel) + the row-split launch */
#define MCD_MH_PATH_SEGMENTS_SPARSE 9         /* sparse likelihood, 3 .. 2048 nodes: the same with the quadratic form updated through the rows of the moved distances (k_mh_segment_sparse.hip); a dense proposal: proposed by the segment before it + the one-launch full form */
int mcd_mh_last_path(const mcd_mh_t* m);
/* LDS bytes per workgroup of the persistent kernel the last mcd_mh_run launched (reporting: a profiler's kernel trace shows the static group
 * segment only, which is 0 for the kernels that size their LDS at launch); 0 when the run took per-step launches only. */
int64_t mcd_mh_last_dynamic_lds(const mcd_mh_t* m);
/* Auto tuning at the end of a tuning period [mcmc]: t' = clamp(t exp(2 (rate - optimal(dim))), 1e-5, 1e3). */
int mcd_mh_tune(mcd_mh_t* m);
/* tune: [batch][n_prop]; accepted / tried: counters since the last mcd_mh_tune / mcd_mh_reset_counters. */
int mcd_mh_get_tuning(const mcd_mh_t* m, double* tune, int32_t* accepted, int32_t* tried);
int mcd_mh_set_tuning(mcd_mh_t* m, const double* tune);
int mcd_mh_reset_counters(mcd_mh_t* m);
/* Reciprocal temperatures beta[batch] in (0, 1] (default 1): chain b accepts with (prior x likelihood)^beta[b], the
 * heated chains of Metropolis-coupled MCMC (`mc3`, app/Main.hs:476-478; package `mcmc`). */
int mcd_mh_set_temperatures(mcd_mh_t* m, const double* beta);
/* The power posterior: exponents beta[batch] in [0, 1]; chain b accepts with prior x likelihood^beta[b], the target of a path point of the
 * marginal-likelihood analysis below (mcd_ml_estimate) -- the likelihood ALONE is heated, and beta = 0 (the prior) is allowed.  The ln
 * acceptance ratio is ((lp1 - lp) + beta (ll1 - ll)) + ln(q-ratio x Jacobian) in this mode; the mode is the handle's: this call sets it,
 * mcd_mh_set_temperatures and mcd_mh_mc3_init set the other one ((prior x likelihood)^beta), and a handle on which this call is never
 * made behaves as before, bit for bit.  Nothing else of a run changes; the recorder keeps storing beta[b] with every sample -- in this
 * mode the likelihood's exponent.  Not-a-number and infinities: a proposal of prior 0 (lp1 = -inf) is rejected; a NaN anywhere in the
 * ratio rejects; beta = 0 with a ln likelihood of the proposal that is not finite gives 0 x inf = NaN and rejects (the prior-only
 * chain does not wander where the likelihood cannot be evaluated).  Refused, the handle untouched: a value outside [0, 1] or a NaN
 * (MCD_ERR_INVALID_ARG); MC3 initialised on the handle (MCD_ERR_UNSUPPORTED).  mcd_mh_record_summary keeps refusing chains whose beta is
 * not 1, in either mode. */
int mcd_mh_set_power(mcd_mh_t* m, const double* beta);
/*
 * The swap phase of Metropolis-coupled MCMC on the device.  Replaces: the swap bookkeeping of `mc3 (MC3Settings (NChains 4)
 * (SwapPeriod 2) (NSwaps 3))`, app/Main.hs:476-478 (package `mcmc`; its initial ladder and ladder tuning are not restated).
 *   mcd_mh_mc3_init   groups of n_chains consecutive GLOBAL chains (total_chains of them over all GPUs, a multiple of n_chains;
 *                     this handle holds [first_chain, first_chain + batch), mcd_mh_set_chain_offset), ladder betas[n_chains]
 *                     (betas[0] = 1, decreasing); chain c starts with rank c mod n_chains; sets this handle's temperatures.
 *   mcd_mh_mc3_swap   one phase: in every group n_swaps distinct adjacent rank pairs, in random order, exchange their
 *                     TEMPERATURES with probability min(1, exp((beta_i - beta_j)(ln pi_j - ln pi_i))), pi = prior x likelihood
 *                     (the states stay where they are: the same Markov chain, 8 bytes per chain on the wire).  gathered =
 *                     device pointer [world][3][chains_per_rank], what mcd_shard_allgather makes of the ranks'
 *                     mcd_mh_posterior_device arrays; NULL when the handle holds every chain.  Every rank evaluates all
 *                     groups from the gathered values with Philox numbers keyed (seed, group, phase): all ranks hold the same
 *                     table and the run does not depend on the number of GPUs.  Enqueued on the sampler's stream.
 *   mcd_mh_mc3_get    rank[total_chains], swap counters tried / accepted[n_chains - 1] per rung, beta[batch] (any may be NULL).
 * One period of the reference's loop = mcd_mh_run (SwapPeriod iterations) -> mcd_shard_allgather of the posterior on the
 * sampler's stream -> mcd_mh_mc3_swap; monitors read the chains whose rank is 0.
 */
int mcd_mh_mc3_init(mcd_mh_t* m, int n_chains, const double* betas, int64_t total_chains, uint64_t seed);
int mcd_mh_mc3_swap(mcd_mh_t* m, int n_swaps, const double* gathered, int world, int64_t chains_per_rank);
int mcd_mh_mc3_get(const mcd_mh_t* m, int32_t* rank, int64_t* tried, int64_t* accepted, double* beta);
/* age_sum / age_sq: [batch][n_nodes] running sums over *n_samples accumulated iterations; reset with the call below. */
int mcd_mh_get_age_sums(const mcd_mh_t* m, double* age_sum, double* age_sq, int64_t* n_samples);
int mcd_mh_reset_age_sums(mcd_mh_t* m);
/*
 * The chains of one driver become the chains of the other ON THE DEVICE (k_handover.hip): what a host that runs the reference's
 * `--hamiltonian` mode (`maybeHamiltonianProposal`, app/Definitions.hs:272-278; target `getHTarget`, app/Main.hs:349-368; `nutsWith`,
 * app/Hamiltonian.hs:95-105) needs between the Metropolis-Hastings cycle and the NUTS transition, without seven arrays crossing the bus
 * twice per iteration.
 *   mcd_hmc_take_state   h := the current states of m.  Leaves h exactly as mcd_hmc_set_state would after mcd_mh_get_state of the same
 *                        chains: state arrays, position, ln target and gradient (the gradient kernels run at the new point).
 *   mcd_mh_take_state    m := the states h holds.  Leaves m exactly as mcd_mh_set_state would after mcd_hmc_get_state: the state arrays
 *                        and ln prior, ln likelihood, ln jacobianRootBranch from the launches mcd_mh_set_state uses (not h's values, which
 *                        come out of the gradient kernels and are other bits); whatever a later mcd_mh_run derives when it starts -- prior
 *                        blocks, kept summands, the incremental z / q -- is derived from the new states.  Step counter, tuning parameters,
 *                        counters, age sums, recorder and temperatures of m are untouched.
 * One launch each way copies the scalars [5][batch] and the first n_nodes entries of every row of heights and rates (the two handles may
 * have different leading dimensions), lanes over the node index.  The handles own different streams: the taking handle's stream waits for
 * an event of the other's, nothing waits for the whole device, and the host waits where the set_state calls wait (once, at the end).
 * Refused with MCD_ERR_INVALID_ARG, the message naming the mismatch, both handles untouched: different devices, different numbers of
 * nodes or parent arrays, different batches, no state on the source.
 */
int mcd_hmc_take_state(mcd_hmc_t* h, const mcd_mh_t* m);
int mcd_mh_take_state(mcd_mh_t* m, const mcd_hmc_t* h);
/*
 * The Hamiltonian proposal in the cycle: `maybeHamiltonianProposal` (app/Definitions.hs:272-278) adds one NUTS proposal of weight 1
 * (`nutsWith`, app/Hamiltonian.hs:95-105) on the target of `getHTarget` (app/Main.hs:349-368) to the Metropolis-Hastings cycle.
 *   mcd_mh_attach_hamiltonian   from now on every iteration of mcd_mh_run BEGINS with one NUTS transition of every chain on h, and the
 *                        steps_per_iter scheduled proposals follow.  DEVIATION: the reference shuffles the proposal into the cycle anew
 *                        at every iteration, so its position is random there; here it is the first.  What the kernels do at the end of
 *                        an iteration -- recorder store, accumulate, age sums -- therefore sees the complete iteration, and the recorder
 *                        and the summaries work unchanged.  DEFINITION: mcd_mh_run(m, schedule, n_iter, S, ...) gives the bits of, for
 *                        it = 0 .. n_iter - 1: mcd_hmc_take_state(h, m); mcd_hmc_nuts(h, eps, inv_mass, max_depth, seed, the chain
 *                        offset of m, first_transition + done + it, ...); mcd_mh_take_state(m, h); mcd_mh_run(m, schedule + it S, 1, S,
 *                        ...) without an attachment -- `done` the attached transitions since this call, so consecutive runs continue the
 *                        stream.  eps[batch] and inv_mass[dim] are copied to the device once, here; inv_mass == NULL: the dense metric
 *                        set on h (mcd_hmc_set_metric), in whichever form h has.  seed: the caller's (a host that runs both drivers on
 *                        one seed passes seed ^ constant, see mcd_hmc_nuts); the chain offset is m's (mcd_mh_set_chain_offset), so the
 *                        shards of a sharded run keep disjoint streams.  trace_alpha / trace_accept keep their shape and hold the
 *                        scheduled proposals only; mcd_mh_last_path reports the path of the Metropolis-Hastings stretches; the
 *                        recorder's room is one check for the whole call, before anything is launched.  No kernel of either driver
 *                        changes: per iteration the cost beside the transition is two copy launches, one posterior evaluation, and the
 *                        launch boundaries of a run of one iteration.  h must outlive the attachment; mcd_mh_destroy does not destroy it.
 *                        MCD_ERR_UNSUPPORTED, the handles untouched: MC3 initialised on m, m in power-posterior mode, any temperature of
 *                        m other than 1 (a tempered Hamiltonian target is not built) -- and while attached the same from
 *                        mcd_mh_mc3_init, mcd_mh_set_power and mcd_mh_set_temperatures (other than 1).  MCD_ERR_INVALID_ARG: the
 *                        mismatches of mcd_hmc_take_state; an eps that is not positive and finite; max_depth outside what mcd_hmc_nuts
 *                        accepts; an inv_mass that does not fit h's metric (a vector while h has a dense metric, NULL while it has none);
 *                        an active recorder on h; a second attach without detach.  The last three are checked again when a run starts.
 *   mcd_mh_detach_hamiltonian   ends the attachment; the handle then runs what a handle that never had one runs, to the bit.
 *   mcd_mh_hamiltonian_stats    *transitions made since the attach call (or the last reset) and per chain the sums over them of the
 *                        acceptance statistic (the alpha of mcd_hmc_nuts), tree depth, leapfrog steps and divergent transitions,
 *                        added on the device after every transition (no host copy per iteration); any may be NULL; reset != 0 clears them.
 */
int mcd_mh_attach_hamiltonian(mcd_mh_t* m, mcd_hmc_t* h, const double* eps, const double* inv_mass, int max_depth, uint64_t seed,
                              uint64_t first_transition);
int mcd_mh_detach_hamiltonian(mcd_mh_t* m);
int mcd_mh_hamiltonian_stats(const mcd_mh_t* m, int64_t* transitions, double* alpha_sum, int64_t* depth_sum, int64_t* leapfrog_steps,
                             int64_t* divergent, int reset);
/*
 * The sample recorder: thinned samples of every chain kept ON THE DEVICE while mcd_mh_run runs.  Replaces: the `monitor` of
 * app/Definitions.hs:288-417 (`mcmc`'s MonitorFile with period 2 everywhere) as the source of the states that the monitor files and
 * scripts/analyze read -- without cutting the run into calls of one monitor period with a state read-back after each.
 *   mcd_mh_record_begin   a ring of capacity_samples slots on the handle's device; the iteration count starts at 0.  period >= 1,
 *                         capacity_samples >= 1; one recorder per handle (a second begin without end is refused).
 *   mcd_mh_run            while a recorder is active: the state of every chain at the END of every iteration whose number is a multiple of
 *                         period is stored as one sample, by the kernels of whichever launch structure the run takes (all of
 *                         MCD_MH_PATH_*).  Iterations count from mcd_mh_record_begin over consecutive calls, so calls of any lengths give
 *                         the samples of one long call.  A call whose samples do not fit the free slots returns MCD_ERR_INVALID_ARG before
 *                         anything is launched (the message names both numbers) and leaves the handle as it was.  The chains themselves do
 *                         not change: states, posteriors, traces, counters and age sums are the same bits with and without a recorder.
 *                         This host-side check is the contract.  On the device sample number k = iteration / period goes to slot
 *                         (k - 1) mod capacity, so no store can leave the ring; were the host's count ever wrong, the newest sample
 *                         would overwrite the oldest unfetched one (not be dropped).  If a call fails after it has launched
 *                         (MCD_ERR_HIP), the recorder's count no longer matches the chains: end the recorder.
 *   mcd_mh_record_count   samples waiting to be fetched.
 *   mcd_mh_record_fetch   waits for the handle's stream, copies the oldest *n_out = min(waiting, max_samples) samples to the host,
 *                         sample-major, and frees their slots: iteration[n], scalars[n][batch][5] (birth, death, tH, rMu, rVar),
 *                         heights[n][batch][n_nodes], rates[n][batch][n_nodes], post[n][batch][3] (ln prior, ln likelihood, ln
 *                         jacobianRootBranch of the accepted state), beta[n][batch] (the reciprocal temperature the chain had: which chains
 *                         were cold under MC3).  Any of the arrays may be NULL.
 *   mcd_mh_record_end     frees the ring.  mcd_mh_set_state leaves an active recorder and its count alone; mcd_mh_destroy frees it.
 */
int mcd_mh_record_begin(mcd_mh_t* m, int32_t period, int64_t capacity_samples);
int mcd_mh_record_count(const mcd_mh_t* m, int64_t* n_samples);
int mcd_mh_record_fetch(mcd_mh_t* m, int64_t max_samples, int64_t* n_out, int64_t* iteration, double* scalars, double* heights, double* rates,
                        double* post, double* beta);
int mcd_mh_record_end(mcd_mh_t* m);
/*
 * Posterior summaries and convergence diagnostics of a trace, computed on the device (k_summary.hip).  Replaces: the node-age summary of
 * scripts/trees-monitor-summary-ultrametric:149-175 (mean, maximum-likelihood variance, minimum, maximum and the 95 % interval per node)
 * without fetching a sample, and what the reference leaves to Tracer on its one chain: split R-hat and the effective sample size over
 * the lock-step chains.  A trace is n samples x batch chains x q quantities; with l = n batch pooled values, per quantity (pooled[q][9]):
 *   0 mean, 1 variance (/ l; two passes, never sum x^2 - (sum x)^2 / l), 2 minimum, 3 maximum,
 *   4, 5  sorted[i] and sorted[i + m - 1], i = floor(0.025 l), m = floor(0.95 l): EXACT, elements of the input (radix select),
 *   6 split R-hat: the oldest sample is dropped if n is odd, every chain is halved into M = 2 batch sequences of n_h = n / 2 samples;
 *     W = mean of their unbiased variances, Bv = n_h x unbiased variance of their means, var+ = (n_h - 1) / n_h W + Bv / n_h,
 *     rhat = sqrt(var+ / W),
 *   7 effective sample size on the same sequences: gamma_{m,t} = 1 / n_h sum_i (x_i - mean_m)(x_{i+t} - mean_m),
 *     rho_t = 1 - (W - mean_m gamma_{m,t}) / var+, P_k = rho_{2k} + rho_{2k+1}; tau = -1 + 2 sum_k min(P_k, P_{k-1}) while P_k > 0 and
 *     2 k + 1 <= max_lag; tau = max(tau, 1 / log10(M n_h)); ess = M n_h / tau,
 *   8 the last lag that entered that sum (-1: none); equal to max_lag: the cap ended the sum, not Geyer's rule.
 * per_chain[batch][q][4] (may be NULL): mean, unbiased variance (/ (n - 1)), minimum, maximum of every chain.
 * max_lag: odd, 1 .. min(MCD_SUMMARY_MAX_LAG, n_h - 1); 0: no effective sample size (7 and 8 are NaN).  n batch must lie in [2, 2^32).
 * A constant sequence or chain has the variance 0 exactly, whatever the rounding of its mean.
 * A quantity with W = 0 or var+ = 0 (a leaf's age, the root's height) or n_h < 2 has rhat = ess = last lag = NaN.  A NaN anywhere in a
 * quantity makes every output of that quantity NaN and touches no other quantity; +-inf are ordered as numbers; which of -0.0 and +0.0
 * is the smaller is unspecified.  No floating-point atomics and a fixed order of every sum: two calls on the same data return the same bits.
 *   mcd_trace_summary         a plain array X[n][batch][ldq], ldq >= q, on the host (copied) or on device device_id (read in place).
 *   mcd_mh_record_quantities  q = 2 n_nodes + 9 of the call below, in the order: ages tH h_v [n_nodes] (one fp64 multiply), rates
 *                             [n_nodes], birth, death, tH, rMu, rVar, ln prior, ln likelihood, ln jacobianRootBranch,
 *                             ln posterior = (ln prior + ln likelihood) + ln jacobianRootBranch.
 *   mcd_mh_record_summary     waits for the handle's stream and summarises the waiting samples [skip, skip + n_samples) of the recorder
 *                             (n_samples < 0: all after skip; *n_used = their number), read in the ring where they lie -- also where the
 *                             window wraps around its end.  Frees no slot and changes nothing that a later mcd_mh_record_fetch,
 *                             mcd_mh_run or mcd_mh_get_* can see.  Refused before any launch, the handle untouched: no active recorder,
 *                             skip at or beyond the waiting count, a window past it, a bad max_lag (MCD_ERR_INVALID_ARG); MC3 initialised
 *                             on the handle or a temperature other than 1 (MCD_ERR_UNSUPPORTED: under MC3 the temperatures wander
 *                             between the chains, so a chain is not a cold sequence; mcd_mh_record_summary_mc3 below follows a
 *                             temperature through the swaps).
 *   mcd_mh_record_summary_mc3 the same summary of a handle with mcd_mh_mc3_init done, over the RUNG-`rung` SEQUENCES of its G = batch /
 *                             n_chains groups: at every recorded sample exactly one chain of a group ran at ladder[rung] (the recorded
 *                             beta equals it bit for bit), and the sequence is, sample by sample, the record of that chain (k_mc3_summary.hip
 *                             gathers it out of the ring; rung 0 is the cold sequence, what the reference's monitors report).  Columns and
 *                             statistics as above with "chain" read as "a group's rung sequence": pooled[q][9] over l = n G values, split
 *                             R-hat and effective sample size over 2 G half sequences, per_group[G][q][4] (may be NULL).  Optional outputs:
 *                             holder[n][G], the local chain (0 .. n_chains - 1) that carried the rung; visits[batch][n_chains], the samples
 *                             of the window every chain spent at each rung; round_trips[batch], its completed passages cold -> hottest ->
 *                             cold (armed at rung 0, marked at rung n_chains - 1, counted at the next return to rung 0) -- whether the
 *                             ladder mixes, which the swap counters of mcd_mh_mc3_get do not show.  The contract is
 *                             mcd_mh_record_summary's: waits for the stream, reads the window where it lies, frees no slot, changes nothing
 *                             a later call can see, the same bits on every call; the gathered trace is allocated for the call (an
 *                             allocation failure: MCD_ERR_HIP with the byte count).  Refused before any launch, the handle untouched and
 *                             *n_used = 0: what mcd_mh_record_summary refuses as MCD_ERR_INVALID_ARG, with n G in the place of n batch;
 *                             MC3 not initialised; rung outside 0 .. n_chains - 1 (MCD_ERR_INVALID_ARG); a handle whose chains are not
 *                             whole groups, first chain or batch no multiple of n_chains (MCD_ERR_UNSUPPORTED).  A window in which some
 *                             sample of some group does not have exactly one chain at the rung -- recorded before mcd_mh_mc3_init or after
 *                             a mcd_mh_set_temperatures -- is found by the gather: MCD_ERR_INVALID_ARG, the message names one such sample,
 *                             its group and the count, and no output other than *n_used is written.
 */
#define MCD_SUMMARY_COLS 9
#define MCD_SUMMARY_MAX_LAG 255 /* four waves of 64 lags each share one sliding window of 256 + 32 rows in LDS */
int mcd_trace_summary(int64_t n, int64_t batch, int64_t q, int64_t ldq, const double* X, int on_device, int device_id, int32_t max_lag,
                      double* pooled, double* per_chain);
int mcd_mh_record_quantities(const mcd_mh_t* m, int64_t* q);
int mcd_mh_record_summary(mcd_mh_t* m, int64_t skip, int64_t n_samples, int32_t max_lag, int64_t* n_used, double* pooled, double* per_chain);
int mcd_mh_record_summary_mc3(mcd_mh_t* m, int rung, int64_t skip, int64_t n_samples, int32_t max_lag, int64_t* n_used, double* pooled,
                              double* per_group, int32_t* holder, int64_t* visits, int64_t* round_trips);
/*
 * The marginal likelihood ln Z = ln integral prior x likelihood from power-posterior chains, computed on the device (k_marginal.hip).
 * Replaces: `marginalLikelihood mlS p l c m i g` (runMarginalLikelihood, app/Main.hs:511-543; 128 points, app/Definitions.hs:447-472).
 * What package `mcmc` does in detail (its point spacing, its walk along the path forward and backward) is not restated: the definitions
 * below are this library's, and the estimate is unpinned against `mcmc`'s own implementation.
 * Layout: K = n_points path points with the exponents betas[K], betas[0] = 0 < ... < betas[K - 1] = 1.  The chain with the GLOBAL number
 * g (first chain of the handle + b; b itself for a plain array) runs at point g mod K and is replicate g / K; batch and the first chain
 * are multiples of K, so the C = batch / K replicates each hold the whole path (mcd_mh_set_power with beta[b] = betas[g mod K]).
 * With delta_p = betas[p + 1] - betas[p] and x the n ln likelihoods of a chain -- per (point p, replicate r): mean m, M2 = sum (x - m)^2
 * (two passes, never sum x^2 - ...), mx = max x and, for p < K - 1, S = sum exp(delta_p (x - mx)).
 *   point[K][MCD_ML_COLS], pooled over the n C values of a point: 0 mean, 1 unbiased variance, 2 minimum, 3 maximum,
 *     4 ln r_p = delta_p MX + ln(sum_r S_r exp(delta_p (mx_r - MX)) / (n C)), MX the point's maximum (NaN for p = K - 1): the stepping
 *     stone ln E_{beta_p}[likelihood^delta_p] (Xie et al. 2011);
 *   replicate[C][2], from replicate r's chain of every point alone: 0 lnZ_ss_r = sum_p [delta_p mx_{p,r} + ln(S_{p,r} / n)],
 *     1 lnZ_ti_r = sum_p delta_p (m_{p,r} + m_{p+1,r}) / 2 (thermodynamic integration, trapezoid);
 *   out[4]: 0 the pooled stepping-stone estimate sum_p ln r_p, 1 its standard error sd(lnZ_ss_r) / sqrt(C) (unbiased sd), 2 the pooled
 *     trapezoid sum_p delta_p (mean_p + mean_{p+1}) / 2, 3 sd(lnZ_ti_r) / sqrt(C).
 * The replicates are independent chains, so the standard errors hold whatever the autocorrelation inside a chain; C = 1 gives NaN.  The
 * trapezoid carries a discretisation bias that the standard error does not show.  A chain or point whose values are all equal has that
 * value as its mean and the variance 0 exactly; equal replicate estimates give the standard error 0 exactly.  A NaN in a point's values
 * makes that point's columns NaN and every total that uses them NaN.  No floating-point atomics and a fixed order of every sum: two calls
 * on the same data return the same bits.  Limits: 2 <= K <= 4096, n >= 1, n C in [2, 2^32) (MCD_ERR_INVALID_ARG otherwise, as for betas
 * that do not start at 0, end at 1 and increase strictly, or a batch that is no multiple of K).  Any of point / replicate / out may be NULL.
 *   mcd_ml_estimate         a plain array ll[n][batch] on the host (copied) or on device device_id (read in place).
 *   mcd_mh_record_marginal  the waiting samples [skip, skip + n_samples) of the handle's recorder (n_samples < 0: all after skip;
 *                           *n_used = their number), ln likelihood read in the ring where it lies -- also where the window wraps.  The
 *                           contract is mcd_mh_record_summary's: waits for the handle's stream, frees no slot, changes nothing a later
 *                           call can see; window errors (and its limits: n batch < 2^32) and betas errors are refused before any launch,
 *                           the handle untouched and *n_used = 0.  The exponent stored with every (sample, chain) of the window must
 *                           equal betas[g mod K] bit for bit: a window that reaches back before mcd_mh_set_power, or chains run at other
 *                           exponents, is found by the first kernel -- MCD_ERR_INVALID_ARG, the message names one such sample and chain,
 *                           and no output other than *n_used = 0 is written.  The same bits as mcd_ml_estimate on the fetched ln
 *                           likelihoods of the same window.
 */
#define MCD_ML_COLS 5
int mcd_ml_estimate(int64_t n, int64_t batch, const double* ll, int on_device, int device_id, int n_points, const double* betas, double* point,
                    double* replicate, double* out);
int mcd_mh_record_marginal(mcd_mh_t* m, int n_points, const double* betas, int64_t skip, int64_t n_samples, int64_t* n_used, double* point,
                           double* replicate, double* out);

/* ------------------------------------------------------------------------------------------------
 * The sparse form: the precision matrix as it is, in CSR on the device, no densification; N up to MCD_MAX_SPARSE_DIM.
 * Replaces: logDensitySparseMultivariateNormal (app/Probability.hs:178-184) and the closure likelihoodFunction (Sparse mu
 * sigmaInvSparse logDetSigma) (:279) over the operands of getData's SparseS branch (app/Main.hs:95-97: the association list
 * [((i, j), v)] of `prepare`'s graphical-lasso estimate, :142-155, 257-277) -- the reference's route for trees with thousands
 * of branches (tutorial/main/tutorial.org:487-496), beyond MCD_MAX_DIM of the dense kernels.
 *   ll = -N ln sqrt(2 pi) - 1/2 (logdet_sigma + dx^T P dx),  dx = x - mu;   mcd_sparse_grad_batch also returns its gradient
 *   G = -1/2 (P + P^T) dx  (= -P dx for the symmetric matrices `prepare` writes).
 * row / col / val: the nnz entries in any order, entries of one position are added up; P is used as given (no symmetrisation,
 * no positive-definiteness check: the reference evaluates the form with whatever the .data file holds).  Batches are chain-major
 * like everywhere; trees as in mcd_tree_create.  Up to 4096 chains the log-density is ONE launch (a workgroup stages the dx of one or two
 * chains in LDS and walks the flat stream of the matrix's entries; for an exactly symmetric matrix the upper triangle only), beyond that
 * three launches with lanes = chains; the two agree to rounding.  Both samplers take the sparse handle as it is, for trees of 3 .. 2048
 * nodes: the Metropolis-Hastings driver by mcd_mh_create_sparse, the leapfrog / NUTS driver by mcd_hmc_create_sparse over
 * mcd_sparse_tree_grad_batch (nothing is densified; mcd_mvn_create with a densified matrix, N <= MCD_MAX_DIM, is no longer needed for either).
 * mcd_sparse_release_stream: a host that makes short-lived streams calls it before destroying one (the gradient's and the large batches'
 * scratch buffer of that stream is freed; like mcd_mvn_release_stream).
 */
#define MCD_MAX_SPARSE_DIM 8192
typedef struct mcd_sparse mcd_sparse_t;
typedef struct mcd_sparse_tree mcd_sparse_tree_t;
int mcd_sparse_create(mcd_sparse_t** out, int n, const double* mu, int64_t nnz, const int32_t* row, const int32_t* col, const double* val,
                      double logdet_sigma, int device_id);
void mcd_sparse_destroy(mcd_sparse_t* h);
int mcd_sparse_dim(const mcd_sparse_t* h);
int64_t mcd_sparse_nnz(const mcd_sparse_t* h);   /* stored entries after adding up duplicates */
int mcd_sparse_release_stream(const mcd_sparse_t* h, void* stream /* hipStream_t */);
int mcd_sparse_logpdf_batch(const mcd_sparse_t* h, const double* X, int64_t ld, int64_t batch, int on_device, void* stream, double* ll);
int mcd_sparse_grad_batch(const mcd_sparse_t* h, const double* X, int64_t ld, int64_t batch, int on_device, void* stream, double* ll,
                          double* G, int64_t ldg);
/* State -> ln likelihood (likelihoodFunctionWrapper, app/Probability.hs:195-207) and ln jacobianRootBranch (:393-410) over a sparse
 * precision matrix; arguments as mcd_tree_loglik_batch. */
int mcd_sparse_tree_create(mcd_sparse_tree_t** out, const mcd_sparse_t* h, int n_nodes, const int32_t* parent);
void mcd_sparse_tree_destroy(mcd_sparse_tree_t* t);
int mcd_sparse_tree_loglik_batch(const mcd_sparse_tree_t* t, const double* heights, const double* rates, int64_t ld_state, const double* tH,
                                 const double* rMu, int64_t batch, int on_device, void* stream, double* ll, double* log_jac);
/* State -> ln likelihood and its gradient with respect to the state over the sparse precision matrix: arguments and semantics of
 * mcd_tree_grad_batch (g_heights / g_rates [batch][ld_state], every node; g_rates[.][0] = 0), with y = 1/2 (P + P^T) dx in place of the
 * factor sweep.  ONE launch, no scratch buffer, a workgroup per one or two chains (csrc/k_sparse_grad.hip); every sum in an order that the
 * matrix and the tree fix: a chain's outputs are the same bits whatever the batch, the chains per workgroup (mcd_set_option
 * "MCD_SPARSE_GRAD_CHAINS" = 1 | 2) and the kind of pointers.  A chain whose ln likelihood is NaN has NaN in every gradient entry; no
 * other chain is touched.  Trees of 3 .. 2048 nodes (MCD_ERR_UNSUPPORTED beyond).  Device pointers: an output may be its own input array
 * (g_heights = heights, g_rates = rates), not the other one. */
int mcd_sparse_tree_grad_batch(const mcd_sparse_tree_t* t, const double* heights, const double* rates, int64_t ld_state, const double* tH,
                               const double* rMu, int64_t batch, int on_device, void* stream, double* ll, double* g_heights, double* g_rates,
                               double* g_tH, double* g_rMu);
/* The leapfrog / NUTS driver (mcd_hmc_*, above) over that likelihood: an ordinary mcd_hmc_t -- every mcd_hmc_* entry point works on it
 * unchanged; a leapfrog step and a NUTS round are still the two gradient launches + one (the prior gradient, mcd_sparse_tree_grad_batch's
 * launch, k_hmc / k_nuts).  Trees of 3 .. 2048 nodes, the range of mcd_mh_create_sparse (MCD_ERR_UNSUPPORTED beyond); tree and prior on
 * the same device with the same node count (MCD_ERR_INVALID_ARG otherwise); they must outlive the driver. */
int mcd_hmc_create_sparse(mcd_hmc_t** out, const mcd_sparse_tree_t* tree, const mcd_prior_t* prior, int calibrations_available, int64_t batch);

/* ------------------------------------------------------------------------------------------------
 * The graphical lasso of `prepare` on the device (csrc/k_glasso.hip, csrc/glasso_capi.cpp).  Replaces: the glasso call behind
 * `prepare --likelihood-spec "SparseMultivariateNormal rho"` (app/Main.hs:257-276), the step that turns a tree list into the sparse
 * precision matrix of mcd_sparse_create, at the reference's production sizes (tutorial/goe: 2011 branch dimensions).
 *   maximise  ln det Theta - tr(S Theta) - rho ||Theta||_1   (the l1 norm over all entries, or, penalize_diagonal = 0, the off-diagonal ones)
 * by block coordinate descent over the columns of W = Theta^-1 with the lasso sub-problem of a column solved by cyclic coordinate descent
 * and warm starts (Friedman, Hastie, Tibshirani 2008), the algorithm and the unique optimum of mcmc-date_amd/prepare.py: graphical_lasso.
 *   mcd_glasso_components  exact screening, pure host code (no device needed): label[i] = the connected component of variable i in the
 *                          graph {i != j : |S_ij| > rho}, numbered 0 .. *n_components - 1 by their smallest member.  The components are
 *                          the blocks of the optimal Theta (Witten, Friedman, Simon 2011; Mazumder, Hastie 2012).
 *   mcd_glasso             S, W, Theta: host arrays [n][n], row-major.  Every component of two or more variables is one independent problem
 *                          of one workgroup; a singleton is W_ii = S_ii (+ rho), Theta_ii = 1 / W_ii; between components W and Theta are 0.
 *                          One launch is one outer pass over the columns; between launches the host applies graphical_lasso's stopping rule
 *                          max |W - W_old| <= tol max(1, mean |S - diag S|), at most max_iter passes; a column's descent ends at a sweep
 *                          that changes no coefficient by more than tol, at most max_iter sweeps.  Theta is symmetrised and entries below
 *                          1e-14 are set to 0.  Every sum in index order, no atomics: the same input gives the same bits on every call.
 *   info[MCD_GLASSO_INFO_LEN]: 0 outer passes used, 1 converged (0 | 1), 2 number of components, 3 size of the largest component,
 *                          4 coordinate updates over all passes, 5 1: some column's descent stopped at max_iter sweeps, 6 components of two
 *                          or more variables (= workgroups per launch), 7 reserved (0).
 * Refused before any launch (MCD_ERR_INVALID_ARG unless said otherwise): n < 1; rho negative or not finite; tol negative; max_iter < 1; a
 * NULL array; a non-finite entry of S; |S_ij - S_ji| > MCD_GLASSO_SYMMETRY_TOL max(1, |S_ij|, |S_ji|); S_ii <= 0; a component of more than
 * MCD_GLASSO_MAX_DIM variables (MCD_ERR_UNSUPPORTED); then no device (MCD_ERR_NO_DEVICE: no CPU fallback) or a bad device_id.  Reaching
 * max_iter passes without meeting the stopping rule is NOT an error: MCD_OK with info[1] = 0 and the iterate reached.
 */
#define MCD_GLASSO_INFO_LEN 8
#define MCD_GLASSO_MAX_DIM 2048 /* per component: the sparse samplers' limit of 2048 nodes */
#define MCD_GLASSO_SYMMETRY_TOL 1e-10
int mcd_glasso_components(int n, const double* S, double rho, int32_t* label, int32_t* n_components);
int mcd_glasso(int n, const double* S, double rho, int penalize_diagonal, double tol, int max_iter, int device_id, double* W, double* Theta,
               int64_t* info);

/* ------------------------------------------------------------------------------------------------
 * Checkpoint and continue (csrc/ckpt_capi.cpp, csrc/k_checkpoint.hip).  Replaces: `Settings ... Save` and the `continue` command
 * (app/Main.hs:494-509: `mcmc` writes state, tuning, counters, iteration and generator on exit and reloads all of it) and
 * `--init-from-save` (app/Main.hs:424-440: `mhgLoadUnsafe`, state and tuning only).  Between two calls of mcd_mh_run a handle is described
 * by a finite list of arrays and counters, because every run derives its kept quantities afresh when it starts; a blob holds that list.
 * DEFINITION: "one handle, two calls of mcd_mh_run" and "first call, mcd_mh_save, mcd_mh_destroy, the same mcd_mh_create*, mcd_mh_load
 * (MCD_CKPT_FULL), second call" give the same bits on every launch structure (MCD_MH_PATH_*).
 * THE CALLER REBUILDS THE CONFIGURATION, as the reference rebuilds its likelihood closure from <prep>.data at every start: tree,
 * likelihood operands, prior, proposal table, batch, seed, chain offset -- and mcd_mh_record_begin, mcd_mh_mc3_init,
 * mcd_mh_attach_hamiltonian where the saved handle had them.  The blob carries a FINGERPRINT of it: n_nodes, parent[], batch, the
 * likelihood's dimension, dense / sparse, n_prop and every row of the proposal table (the bits of kind, node, n1, n2, jac_root, dim, p0, p1),
 * seed and chain offset.  The likelihood's operands and the prior are NOT hashed: a changed dataset is the caller's to catch, and the saved
 * posterior terms are not re-checked against the rebuilt likelihood.
 * The blob: little-endian 8-byte words; a fixed header (magic, version, header bytes, total bytes, the configuration), a section table of
 * (id, offset, bytes, checksum), a checksum of the header, then the sections (MCD_CKPT_SEC_*), each a multiple of 8 bytes with zero padding.
 * It carries: the state sc[5][batch], heights and rates (n_nodes of every row), post[3][batch] and the prior's blocks [batch][3] AS THEY LIE
 * (never recomputed: on the incremental paths the kept ln likelihood is another rounding of what mcd_mh_set_state would evaluate), the
 * temperatures and the power-posterior bit, tuning parameters and their counters, the age sums with their sample count, the step counter
 * (the random streams' position), the recorder's counts, and, where the handle has them, MC3's rank table, swap counters and phase and the
 * attached Hamiltonian's next transition number, sums, step sizes and inverse masses.  The recorder's ring and an mcd_hmc_t's dense metric
 * (mcd_hmc_get_metric / mcd_hmc_set_metric) are not in it.  Two saves of an untouched handle give the same bytes.
 *   mcd_mh_save_size   *bytes of the blob mcd_mh_save would write now: 8 (17 + 4 S) header bytes for S sections + 384 + 8 (12 B + 4 B n_nodes
 *                      + B P + 2 ceil(B P / 2)) for B chains and P proposals (S = 12); MC3 adds 8 (ceil(total / 2) + 2 (n_chains - 1)) and
 *                      S + 3, an attachment 8 (5 B [+ dim]) and S + 2 [+ 1].
 *   mcd_mh_save        ONE launch gathers every section into a staging blob on the device and forms its checksum (k_ckpt_pack), ONE copy
 *                      brings it to buf; the chains do not change (a handle that saved runs the bits of one that did not).  cap too small:
 *                      MCD_ERR_INVALID_ARG, the needed size in the message and in *written.  Samples waiting in the recorder's ring: refused
 *                      (MCD_ERR_INVALID_ARG; fetch them with mcd_mh_record_fetch first); so is a handle without a state.
 *   mcd_mh_load        flags = MCD_CKPT_FULL: the fingerprint must match; every array and counter above is restored and the handle has a
 *                      state without mcd_mh_set_state.  A handle with an active recorder of the blob's period continues its period phase
 *                      (another period is refused; a handle without a recorder ignores the counts).  A blob with MC3 needs mcd_mh_mc3_init
 *                      done with the same n_chains, total, ladder and seed, a blob with an attachment an attachment of the same max_depth,
 *                      seed and inv_mass presence; either without the other is refused.
 *                      flags = MCD_CKPT_STATE_TUNING (`--init-from-save`): only n_nodes, topology, batch and n_prop must match; state,
 *                      posterior terms and tuning parameters are taken, the tuning counters zeroed; step counter, seed, temperatures, sums,
 *                      recorder, MC3 and attachment stay the handle's own.
 *                      One copy to the device, a launch that recomputes every section's checksum (k_ckpt_verify), and only when the host
 *                      found them equal the launch that scatters the sections (k_ckpt_unpack): EVERY refusal leaves the handle untouched,
 *                      MCD_ERR_INVALID_ARG with the mismatch named in mcd_last_error() -- bad magic, a truncated buffer, len other than the
 *                      blob's total bytes, an unknown version, a failed checksum, a configuration that differs.
 *   mcd_ckpt_inspect   pure host code, no device needed: the header of a blob, after the checks above and every section's checksum.
 *   mcd_ckpt_checksum  the checksum of n_words 8-byte words: sum_i mix(w_i XOR (i + 1) 0x9E3779B97F4A7C15) mod 2^64, mix the splitmix64
 *                      finaliser; the host restatement of what the kernels add up with integer atomics (any order, the same word).
 */
#define MCD_CKPT_FULL 0
#define MCD_CKPT_STATE_TUNING 1
#define MCD_CKPT_MAX_SECTIONS 24
#define MCD_CKPT_FLAG_DENSE 1u
#define MCD_CKPT_FLAG_MC3 2u
#define MCD_CKPT_FLAG_HAMILTONIAN 4u
#define MCD_CKPT_FLAG_INV_MASS 8u
#define MCD_CKPT_FLAG_RECORDER 16u
#define MCD_CKPT_FLAG_POWER 32u
#define MCD_CKPT_SEC_META 1        /* 48 words: the counters the handle keeps on the host */
#define MCD_CKPT_SEC_SC 2          /* [5][batch] birth, death, tH, rMu, rVar */
#define MCD_CKPT_SEC_HEIGHTS 3     /* [batch][n_nodes] */
#define MCD_CKPT_SEC_RATES 4       /* [batch][n_nodes] */
#define MCD_CKPT_SEC_POST 5        /* [3][batch] */
#define MCD_CKPT_SEC_PCOMP 6       /* [batch][3] */
#define MCD_CKPT_SEC_BETA 7        /* [batch] */
#define MCD_CKPT_SEC_TUNE 8        /* [batch][n_prop] */
#define MCD_CKPT_SEC_ACCEPTED 9    /* [batch][n_prop] int32 */
#define MCD_CKPT_SEC_TRIED 10      /* [batch][n_prop] int32 */
#define MCD_CKPT_SEC_AGE_SUM 11    /* [batch][n_nodes] */
#define MCD_CKPT_SEC_AGE_SQ 12     /* [batch][n_nodes] */
#define MCD_CKPT_SEC_MC3_RANK 13   /* [total] int32 */
#define MCD_CKPT_SEC_MC3_TRIED 14  /* [n_chains - 1] int64 */
#define MCD_CKPT_SEC_MC3_ACCEPTED 15
#define MCD_CKPT_SEC_HAM_SUMS 16   /* [4][batch]: alpha (double), depth, leapfrog steps, divergent (int64) */
#define MCD_CKPT_SEC_HAM_EPS 17    /* [batch] */
#define MCD_CKPT_SEC_HAM_INV_MASS 18 /* [dim] */
typedef struct mcd_ckpt_info {
    int32_t version, n_sections;
    int64_t header_bytes, total_bytes;
    uint32_t flags; /* MCD_CKPT_FLAG_* */
    int32_t n_nodes, n_prop, dim, dense;
    int64_t batch, chain0;
    uint64_t seed, step;
    uint64_t topology, table, fingerprint; /* hashes of parent[], of the proposal table, of the whole configuration */
    int32_t section_id[MCD_CKPT_MAX_SECTIONS];
    int64_t section_offset[MCD_CKPT_MAX_SECTIONS], section_bytes[MCD_CKPT_MAX_SECTIONS];
    uint64_t section_checksum[MCD_CKPT_MAX_SECTIONS];
} mcd_ckpt_info_t;
int mcd_mh_save_size(const mcd_mh_t* m, int64_t* bytes);
int mcd_mh_save(mcd_mh_t* m, void* buf, int64_t cap, int64_t* written);
int mcd_mh_load(mcd_mh_t* m, const void* buf, int64_t len, int flags);
int mcd_ckpt_inspect(const void* buf, int64_t len, mcd_ckpt_info_t* info);
uint64_t mcd_ckpt_checksum(const void* words, int64_t n_words);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU.  Chains are independent: every rank (one process per GPU) holds the operands and evaluates its own
 * contiguous block of chains; nothing is exchanged on the likelihood path.  The sampler-level exchange -- the per-chain ln
 * posterior that MC3's swap phase compares (`mc3 (MC3Settings (NChains 4) (SwapPeriod 2) (NSwaps 3))`, app/Main.hs:476-478; in
 * the reference an in-process matter of `mcmc`), diagnostics -- is ONE all-gather per swap period:
 *   mcd_shard_allgather   recv[r * count + i] = send of rank r, element i; device pointers, enqueued on `stream`
 *                         (RCCL ncclAllGather over xGMI; a few KB per rank, latency bound -- no ring of small sends);
 *   mcd_mh_posterior_device  the sampler's device-resident [3][batch] ln prior / ln likelihood / ln Jacobian, what to send.
 * RCCL is loaded at run time; the communicator is made by the wrappers below, so that a host in the reference's language
 * needs no RCCL binding: rank 0 draws an id (mcd_shard_unique_id), hands its MCD_SHARD_ID_BYTES bytes to the other ranks'
 * processes by its own means, every rank calls mcd_shard_comm_create (collective: returns when all ranks have called).
 */
#define MCD_SHARD_ID_BYTES 128
int mcd_shard_unique_id(char id[MCD_SHARD_ID_BYTES]);
int mcd_shard_comm_create(void** comm, int world_size, int rank, const char id[MCD_SHARD_ID_BYTES], int device_id);
void mcd_shard_comm_destroy(void* comm);
int mcd_shard_comm_count(void* comm, int* n_ranks);   /* the rank count the RCCL communicator itself reports (ncclCommCount) */
int mcd_shard_allgather(void* comm, const double* send, double* recv, int64_t count, void* stream);
int mcd_mh_posterior_device(const mcd_mh_t* m, const double** post, void** stream);

#ifdef __cplusplus
}
#endif
#endif /* MCMCDATE_MVN_H */
