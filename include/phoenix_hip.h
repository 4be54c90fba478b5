/*
 * phoenix_hip.h -- C ABI of the MI355X-native PHOENIX NeuralODE engine (libphoenix_hip.so).
 *
 * The reference (QuackenbushLab/phoenix) is pure Python and has NO plugin / FFI interface; its
 * boundary for this path is the Python pair
 *     odeint(func, y0, t, rtol, atol, method, options)           torchdiffeq/_impl/odeint.py:30
 *     odeint_adjoint(...)                                          torchdiffeq/_impl/adjoint.py:165
 * plus the `func(t, y)` protocol implemented by ODENet (odenet.py:85-98).  This header is the
 * native boundary a maintainer binds *underneath* those two functions (INTEGRATION.md shows the
 * ctypes stub); phoenix_amd/ is exactly such a binding.  Each entry point names the reference
 * code it replaces.  All paths are relative to /root/reference/ode_net/code/.
 *
 * Conventions
 *  - plain pointers + sizes; every data pointer is a DEVICE pointer unless marked HOST.
 *  - the caller owns all memory (parameters, states, outputs, workspace); the library never
 *    allocates or frees device memory and keeps no pointer past the call.
 *  - `stream` is a hipStream_t passed as void*; all work is enqueued on it; no call synchronises.
 *  - every function returns a phx_status (0 = enqueued OK).  Solver-level failures (the
 *    reference's AssertionErrors) are reported per trajectory in the `status` output array.
 *  - fp32 state, fp64 time scalars, exactly like the reference (rk_common.py:115-131).
 */
#ifndef PHOENIX_HIP_H
#define PHOENIX_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PHX_ABI_VERSION 7

/* ODENet parameters (odenet.py:42-82), gene-contiguous: every matrix is [rows, N] row-major.
 *   Ws  [H, N]   net_sums.linear_out.weight            (reference layout as is)
 *   Wp  [H, N]   net_prods.linear_out.weight           (reference layout as is)
 *   WaT [2H, N]  net_alpha_combine.linear_out.weight TRANSPOSED (reference stores [N, 2H])
 *   bs, bp [H]   biases;   g [N] gene_multipliers ([1,N] in the reference)                  */
typedef struct phx_params {
    const float *Ws, *bs, *Wp, *bp, *WaT, *g;
    int N, H;
    const void *wimg; /* optional: LDS weight images of THESE parameter values, made by phx_pack_weight_images; the solve
                         entry points then skip their per-launch packing kernel.  NULL: packed per launch. */
} phx_params;

/* Gradient buffers with the same shapes/layouts; the engine ACCUMULATES (+=) into them, or -- overwrite != 0 -- writes
 * them (=): the buffers may then be uninitialised (saves the caller a zero fill). */
typedef struct phx_grads {
    float *Ws, *bs, *Wp, *bp, *WaT, *g;
    int overwrite;
    float *Wa; /* optional (ABI 6): non-NULL = the gradient of net_alpha_combine.linear_out.weight is written HERE in the
                  reference's own layout [N, 2H] (what autograd hands the optimizer, odenet.py:57-60) and WaT is not
                  touched (may be NULL): the caller needs no transposed copy of the 2HN floats afterwards. */
} phx_grads;

/* torchdiffeq SOLVERS entries on the BASELINE path (odeint.py:14-27) */
enum phx_method { PHX_EULER = 0, PHX_MIDPOINT = 1, PHX_RK4 = 2 /* 3/8 rule */, PHX_DOPRI5 = 3 };

/* step control of a batch */
enum phx_control {
    PHX_CTRL_SHARED = 0,        /* reference odeint on y0[B,1,N]: one controller, rms over B*N */
    PHX_CTRL_PER_TRAJECTORY = 1 /* reference training loop: B independent odeint calls        */
};

enum phx_status {
    PHX_OK = 0,
    PHX_ERR_MAX_STEPS = 1,    /* AssertionError 'max_num_steps exceeded'        rk_common.py:154 */
    PHX_ERR_DT_UNDERFLOW = 2, /* AssertionError 'underflow in dt'               rk_common.py:175 */
    PHX_ERR_NONFINITE = 3,    /* AssertionError 'non-finite values in state y'  rk_common.py:176 */
    PHX_ERR_BAD_ARG = 4,
    PHX_ERR_WORKSPACE = 5,    /* workspace too small */
    PHX_ERR_LAUNCH = 6,       /* HIP launch failure */
    PHX_ERR_SYNC_TIMEOUT = 7  /* in-kernel grid barrier timed out (kernel aborted itself) */
};

typedef struct phx_solve_opts {
    int method;         /* phx_method */
    int control;        /* phx_control */
    double rtol, atol;  /* odeint defaults 1e-7 / 1e-9 (odeint.py:30) */
    int t_per_sample;   /* 0: t is [T] shared;  1: t is [B, T] (training loop: t[b] = (t_i, t_{i+1})); with PHX_CTRL_SHARED
                           and calls > 1 (phx_odeint only): t is [calls, T], one grid per call */
    int t_is_f32;       /* 1: the caller's t tensor was float32 (fixed-grid dt is then formed in fp32);
                           2: ... and the buffer passed as `t` still holds float32 values (no conversion) */
    long long max_num_steps; /* <=0: 2^31-1 like the reference (rk_common.py:110) */
    int calls;          /* phx_odeint with PHX_CTRL_SHARED only; > 1: the B rows are `calls` independent odeint calls of
                           B/calls rows each (rows of a call contiguous), every call under its own shared step
                           controller -- the loop of find_gene_influences.py:64-77 in one launch.  0/1: one call.
                           The adjoint entry point ignores it. */
    int ws_keep;        /* ABI 6.  0: the workspace may hold anything -- the call zero-fills its exchange buffers first (6-24 MB
                           at breast scale, on `stream`, in front of the kernel).  1: the caller vouches that the PREVIOUS
                           call that used this workspace was this same entry point with the same shape and options, is
                           ordered before this one on `stream`, returned PHX_OK, and that nothing else wrote to the
                           workspace since: kernels that keep two alternating sets of exchange buffers (the third-generation
                           solve kernels) then skip the fill and clean the idle set themselves; every other kernel fills
                           as with 0.  A first call on a workspace, or one after a shape change, must pass 0. */
} phx_solve_opts;

int phx_abi_version(void);
const char *phx_status_string(int status);
/* number of CUs the engine sizes its persistent grids for (0 if no device) */
int phx_device_cus(void);

/* Workspace size (bytes) for one call of entry point `op` with this shape. */
enum phx_op { PHX_OP_RHS_FORWARD = 0, PHX_OP_RHS_VJP = 1, PHX_OP_ODEINT = 2, PHX_OP_ADJOINT = 3 };
size_t phx_workspace_bytes(int op, int N, int H, int B, int T);
/* Weight images for phx_params.wimg: the per-gene-block LDS layout of the MFMA solve kernels depends only on (N, H), so
 * a caller that runs several solves with the same parameter values (forward + backward of a training step, a validation
 * loop, an analysis scan) packs once.  phx_weight_image_bytes: buffer size (0: this shape has no MFMA plan). */
size_t phx_weight_image_bytes(int N, int H);
int phx_pack_weight_images(const phx_params *p, void *wimg, void *stream);
/* ABI 6: the whole engine layout of one parameter version in ONE kernel, straight from the tensors the reference's
 * ODENet holds (odenet.py:42-82): Ws, Wp [H, N], Wa = net_alpha_combine.linear_out.weight as PyTorch stores it [N, 2H],
 * g [N].  Writes WaT_out [2H, N] (phx_params.WaT) and, when `wimg_out` is non-NULL (phx_weight_image_bytes(N, H) bytes),
 * the packed weight images (phx_params.wimg).  Replaces a transposed copy + phx_pack_weight_images per optimizer step. */
int phx_layout_params(const float *Ws, const float *Wp, const float *Wa, const float *g, int N, int H, float *WaT_out,
                      void *wimg_out, void *stream);
/* ... for phx_odeint with opts->calls = calls (0: this batch of calls cannot be planned, solve the calls one by one) */
size_t phx_odeint_calls_workspace_bytes(int N, int H, int B, int T, int calls);
/* Calls with a time grid of their own: phx_odeint with PHX_CTRL_SHARED, opts->calls = calls > 1 AND opts->t_per_sample = 1
 * takes t as [calls, T], row g the grid of call g (rows [g * B/calls, (g + 1) * B/calls) of y0 / sol / status); a row may
 * increase or decrease whatever its neighbours do, opts->t_is_f32 = 2 holds as for any t.  The loop of validation()
 * (train_insilico.py:77-106: one odeint per validation item over that item's own times) in a few launches.  A call that
 * fails (status != 0 on all of its rows, NaN in the outputs it never reached) does not touch the other calls.  dopri5
 * runs on k1_solve_fwd3 / k1_solve_fwd3c where they plan one call (batch group g = call g), every other case on
 * k1_solve_fwd; a launch takes as many calls as have all their workgroups resident (TG * G <= CUs), the shared chunk
 * driver walks the rest.  calls <= 1 with t_per_sample under shared control stays PHX_ERR_BAD_ARG, and so does any
 * t_per_sample under shared control in phx_odeint_stepped with a step size and in the backward entry points.
 * phx_odeint_calls_grids_workspace_bytes: the workspace of that form (0: no kernel plans a call of B/calls rows -- more
 * than 256 rows of dopri5 beyond the first-generation kernel's 512, PHX_ENGINE=v0: solve the calls one by one).  Unlike
 * phx_odeint_calls_workspace_bytes it depends on the method, and it sizes for 256 CUs when no device is visible. */
size_t phx_odeint_calls_grids_workspace_bytes(int N, int H, int B, int T, int calls, int method);
/* In-silico knockouts (additive, ABI 7): phx_odeint with PHX_CTRL_SHARED, opts->calls = calls >= 1, opts->t_per_sample = 1
 * and t as [calls, T], where call k integrates with gene clamp_gene[k] (DEVICE, [calls]) held at its initial value:
 *     d y[:, clamp_gene[k]] / dt = 0      for the whole time course of call k.
 * The RHS is f = relu(g) (W_alpha z - y) (odenet.py:85-91), so the clamped call IS the solve of the model whose g[gene]
 * is 0, arithmetic included: the sweeps of k1_solve_fwd3 / k1_solve_fwd3c read relu(g) of that gene as 0, and stage
 * slopes, error norm, initial step, FSAL, accept pass and dense output follow from it.  An entry no gene has (negative,
 * >= N) clamps nothing; the list is not validated.  Level 0 in y0 is a knockout, a high level an over-expression.
 * Served only where dopri5 plans the calls on k1_solve_fwd3 / k1_solve_fwd3c (the planning of
 * phx_odeint_calls_grids_workspace_bytes); a batch of more calls than one launch holds goes through the shared chunk
 * driver, list, time rows and y0 / sol rows offset together.
 * PHX_ERR_BAD_ARG before any device call: null clamp_gene (or any pointer phx_odeint refuses), a method other than
 * dopri5, control != PHX_CTRL_SHARED, t_per_sample == 0, calls < 1, B % calls, and a shape whose
 * phx_odeint_clamped_workspace_bytes is 0 (the first-generation kernel would serve it, PHX_ENGINE=v0: solve the calls
 * one by one with g[gene] zeroed).  The size query plans for 256 CUs when no device is visible. */
size_t phx_odeint_clamped_workspace_bytes(int N, int H, int B, int T, int calls);
int phx_odeint_clamped(const phx_params *p, const float *y0, const double *t, int B, int T, const phx_solve_opts *opts,
                       const int *clamp_gene, float *sol, int *status, int *nfe, int *nsteps, void *workspace,
                       size_t workspace_bytes, void *stream);
/* Combination knockouts (additive, ABI 7): phx_odeint_clamped with a SET of held genes per call.  clamp_genes is DEVICE,
 * [calls, width] row-major, 1 <= width <= PHX_CLAMP_MAX: call k holds every gene of its row at its initial value for the
 * whole time course -- exactly the solve of the model whose g is 0 on the set, arithmetic included (the sweeps compare a
 * gene against the call's row, which a workgroup reads once, instead of against one index).  Entries no gene has
 * (-1, >= N) match nothing and pad a shorter set; a gene named twice counts once; the list is not validated.  Planning,
 * refusals and workspace (phx_odeint_clamped_workspace_bytes) are phx_odeint_clamped's, which is the width = 1 case; a
 * batch that spans several launches has its list offset by width x calls together with the time rows and the y0 / sol
 * rows.  PHX_ERR_BAD_ARG before any device call also for width < 1, width > PHX_CLAMP_MAX and a null list. */
#define PHX_CLAMP_MAX 4
int phx_odeint_clamped_sets(const phx_params *p, const float *y0, const double *t, int B, int T, const phx_solve_opts *opts,
                            const int *clamp_genes, int width, float *sol, int *status, int *nfe, int *nsteps,
                            void *workspace, size_t workspace_bytes, void *stream);
/* Perturbation time courses to TRAIN on (additive, ABI 7): a held set per trajectory ROW, forward and adjoint, under
 * PHX_CTRL_PER_TRAJECTORY (t [T], or [B, T] with t_per_sample).  clamp_genes is DEVICE, [B, width] row-major,
 * 1 <= width <= PHX_CLAMP_MAX: row b of y0 holds every gene of row b of the list for its whole time course, the empty set
 * (all entries -1) being an unperturbed sample.  Definition, arithmetic included: row b is solved with the model whose g
 * is 0 on its set -- forward d y[b, k] / dt = 0 on the set; backward the continuous adjoint of that per-row model:
 * q = a relu(g) and k_y are 0 at a held gene, a[k] still evolves (adj_y0[b, k] is dL/d(level the gene is held at)), and
 * g[k] and row k of W_alpha receive nothing from that row.  grads (+)= the sum over the rows, under phx_grads.overwrite
 * like phx_odeint_adjoint_backward.  The parameters are never modified.  Entries no gene has (-1, >= N) match nothing
 * and pad a set; the list is not validated on the device.
 * Served by the CLAMP forms of k1_solve_fwd3 and k1_solve_adj3 (H <= 48; the backward launch runs without the tail
 * kernel); a batch of more rows than one launch holds goes through the shared chunk driver, the list offset by
 * width x rows together with the y0 / sol / t rows.  phx_odeint_clamped_rows_workspace_bytes (op = PHX_OP_ODEINT or
 * PHX_OP_ADJOINT) is 0 exactly where the launch is not served -- H > 48, PHX_ENGINE=v0, a shape the narrow kernels do not
 * plan -- and plans for 256 CUs when no device is visible.  Both entry points return PHX_ERR_BAD_ARG before any device
 * call for a null list (or any pointer the unclamped entry point refuses), width < 1, width > PHX_CLAMP_MAX, a method
 * other than dopri5, control other than PHX_CTRL_PER_TRAJECTORY, and a shape whose size query is 0: solve such batches
 * group by group with g zeroed on each set. */
size_t phx_odeint_clamped_rows_workspace_bytes(int op, int N, int H, int B, int T);
int phx_odeint_clamped_rows(const phx_params *p, const float *y0, const double *t, int B, int T, const phx_solve_opts *opts,
                            const int *clamp_genes, int width, float *sol, int *status, int *nfe, int *nsteps,
                            void *workspace, size_t workspace_bytes, void *stream);
int phx_odeint_adjoint_backward_clamped_rows(const phx_params *p, const double *t, int B, int T, const phx_solve_opts *opts,
                                             const int *clamp_genes, int width, const float *y_saved, const float *grad_y,
                                             float *adj_y0, const phx_grads *grads, int *status, int *nfe, int *nsteps,
                                             void *workspace, size_t workspace_bytes, void *stream);
/* diagnostic: the first launch of such a batch, planned for 256 CUs when no device is visible.  plan[8] = {kernel id (3),
 * HALF form, SPLIT form, rows per launch, launches, batch groups TG, gene-tile groups G, trajectory tiles per group};
 * returns 0 (plan zeroed) where the size query is 0. */
int phx_debug_clamped_rows_plan(int op, int N, int H, int B, int T, int *plan);

/* Replaces ODENet.forward / prior_only_forward (odenet.py:85-98): out[B,N] = f(y[B,N]). */
int phx_rhs_forward(const phx_params *p, const float *y, float *out, int B, int prior_only,
                    void *workspace, size_t workspace_bytes, void *stream);

/* Replaces torch.autograd.grad through ODENet.forward (adjoint.py:116-119; and the autograd
 * backward of prior_only_forward, train_insilico.py:134-138):
 *   vjp_y[B,N] = cot^T df/dy   (overwritten; may be NULL)
 *   grads     += cot^T df/dtheta summed over B  (may be NULL)
 *   f_out[B,N] = f(y)          (may be NULL)                                               */
int phx_rhs_vjp(const phx_params *p, const float *y, const float *cot, float *vjp_y,
                const phx_grads *grads, float *f_out, int B, int prior_only, void *workspace,
                size_t workspace_bytes, void *stream);

/* Replaces odeint(ODENet, y0, t, rtol, atol, method) (odeint.py:30-74; solvers.py:23-30,77-95;
 * rk_common.py:39-228; fixed_grid.py:6-38; dopri5.py; misc.py:47-103; interp.py).
 *   y0 [B,N]; t (double) [T] or [B,T] increasing or decreasing; sol [T,B,N] (sol[0] = y0).
 *   status [B] (int, phx_status per trajectory), nfe [B] (int, RHS evaluations), nsteps [B].
 *   Outputs a failed trajectory (status != 0) never reached are set to NaN.                    */
int phx_odeint(const phx_params *p, const float *y0, const double *t, int B, int T,
               const phx_solve_opts *opts, float *sol, int *status, int *nfe, int *nsteps,
               void *workspace, size_t workspace_bytes, void *stream);

/* Replaces OdeintAdjointMethod.backward (adjoint.py:32-162):
 *   y_saved [T,B,N] forward outputs, grad_y [T,B,N] cotangents of every output time,
 *   adj_y0 [B,N] (overwritten) = dL/dy0,   grads += dL/dtheta (summed over B).
 * The parameter gradient is integrated as a quadrature with the solver's own weights (identical
 * mathematics to the reference's P-sized augmented state, adjoint.py:86-87,127); the adaptive
 * controller's norm covers the [t, y, adj_y] blocks (the reference also includes theta).      */
int phx_odeint_adjoint_backward(const phx_params *p, const double *t, int B, int T,
                                const phx_solve_opts *opts, const float *y_saved,
                                const float *grad_y, float *adj_y0, const phx_grads *grads,
                                int *status, int *nfe, int *nsteps, void *workspace,
                                size_t workspace_bytes, void *stream);

/* options={"step_size": h} of the fixed-grid methods (FixedGridODESolver, solvers.py:36-103): phx_odeint with sub-steps.
 * Euler / midpoint / rk4 step along ONE grid per trajectory, g_k = k * h + t[0] for k < ceil((t[T-1] - t[0]) / h + 1),
 * the last point set to t[T-1], formed in the dtype of the caller's t (opts->t_is_f32); output j is the state at the
 * grid point equal to t[j], else the linear interpolant of the step that passes t[j].  Intermediate states stay on chip.
 * nsteps [B] = grid steps taken, nfe = stages * nsteps.  step_size <= 0 (or not finite), or method dopri5: exactly
 * phx_odeint.  opts->max_num_steps > 0 is a budget of grid steps per trajectory (PHX_ERR_MAX_STEPS in status).
 * PHX_ERR_BAD_ARG when no kernel with the sub-step loop plans the shape (opts->calls > 1, or a shape only the VALU
 * engine serves, H > 256: never one step per interval in silence).  Same workspace as phx_odeint. */
int phx_odeint_stepped(const phx_params *p, const float *y0, const double *t, int B, int T,
                       const phx_solve_opts *opts, float *sol, int *status, int *nfe, int *nsteps,
                       void *workspace, size_t workspace_bytes, void *stream, double step_size);

/* ... and the backward solve under it (adjoint.py:137-154 calling odeint per interval with adjoint_options): every
 * interval [t[i], t[i-1]] has its own grid anchored at t[i] whose last step ends on t[i-1] (no interpolation), one set
 * of quadrature weights per sub-step, the jump after the last one.  nsteps / nfe add up the intervals.  step_size <= 0
 * or dopri5: exactly phx_odeint_adjoint_backward.  opts->max_num_steps > 0 is a budget of grid steps per interval.
 * k1_solve_adj2 and k1_solve_adj have the loop; PHX_ERR_BAD_ARG for a shape only the VALU engine serves (H > 256). */
int phx_odeint_adjoint_backward_stepped(const phx_params *p, const double *t, int B, int T,
                                        const phx_solve_opts *opts, const float *y_saved,
                                        const float *grad_y, float *adj_y0, const phx_grads *grads,
                                        int *status, int *nfe, int *nsteps, void *workspace,
                                        size_t workspace_bytes, void *stream, double step_size);

/* Backward pass of `odeint` itself with a fixed-grid method (torchdiffeq/_impl/odeint.py:30-74 returns an autograd-tracked
 * solution): backpropagation through the solver's own euler / midpoint / rk4 steps (fixed_grid.py:6-38, rk_common.py:96-103),
 * i.e. the DISCRETE adjoint -- the exact gradient of the numbers phx_odeint / phx_odeint_stepped produced, whatever the
 * step.  NOT the continuous adjoint of phx_odeint_adjoint_backward, from which it differs at O(1) for one unconverged step
 * per interval.  Arguments as phx_odeint_adjoint_backward_stepped: y_saved [T,B,N] forward outputs, grad_y [T,B,N], adj_y0
 * [B,N] (overwritten), grads (+= or =, summed over B), status / nfe / nsteps [B], caller-owned workspace.
 *   step_size <= 0: the grid is t itself; the start state of step i is y_saved[i]; grid_steps is ignored.
 *   step_size > 0:  the grid of phx_odeint_stepped (one per trajectory, anchored at t[0], last step clipped, outputs between
 *     grid points linearly interpolated: an output at fraction th of step k hands (1 - th) grad_y to grid state k and
 *     th grad_y to grid state k + 1).  The kernel re-runs the forward grid from y_saved[0], keeps the start state of every
 *     step in the checkpoint region of the workspace ([grid_steps][rows of a launch][N] floats) and sweeps back over them.
 *     grid_steps >= the largest number of grid steps of any trajectory (PHX_ERR_WORKSPACE in status for one with more).
 *   opts->max_num_steps > 0: the forward call's budget of grid steps per trajectory (PHX_ERR_MAX_STEPS in status).
 *   nsteps [B] = grid steps swept back; nfe [B] = RHS evaluations and RHS vector-Jacobian products together: per grid
 *   step s - 1 evaluations that rebuild the stage inputs and s products (2 s - 1), plus the s of the forward re-run under a
 *   step size (3 s - 1), s = stages of the method.
 * One persistent launch (k1_solve_bp) per chunk of the batch plus the gradient reduction.  Served: H <= 128.
 * PHX_ERR_BAD_ARG before any device call: null pointers, non-positive sizes, method dopri5 (no backpropagation through
 * adaptive steps), step_size > 0 with grid_steps < 1; PHX_ERR_BAD_ARG also for a shape no kernel plans (H > 128,
 * PHX_ENGINE=v0); PHX_ERR_WORKSPACE when workspace_bytes < phx_odeint_backprop_workspace_bytes(N, H, B, T, grid_steps).
 *
 * phx_odeint_backprop_workspace_bytes(N, H, B, T, K) = phx_odeint_backprop_workspace_bytes(N, H, B, T, 0)
 *     + 256 * ceil(K * Bc * N * 4 / 256),   Bc = rows of the call's largest launch (B when
 * phx_debug_backprop_launches(N, H, B, T, method) == 1, else the chunk the shared driver walks the batch in); 0: no kernel
 * plans the shape.  Sized for 256 CUs when no device is visible.  K = 0 when the call has no step size.
 * phx_debug_backprop_kernel_m: 5 = k1_solve_bp serves the shape, 0 = refused.  phx_debug_backprop_launches: launches of
 * that kernel one call makes (0: refused).
 * phx_debug_backprop_plan: the launch geometry of the FIRST launch of the batch, plan[0..7] = HT (hidden tiles of 16 rows),
 * NB (gene blocks of 32 a workgroup keeps in LDS), G (workgroups that share one trajectory tile = ceil(nblk / NB)), TG (batch
 * groups), ntg (trajectory tiles of 16 per group), nblk, chunk_rows (rows per launch) and launches.  Returns 1 with a plan,
 * 0 without one (plan zeroed: dopri5, H > 128, PHX_ENGINE=v0).  cus <= 0: the CU count of the current device; a positive
 * `cus` plans for that many CUs and needs no device.  TG * G <= cus always. */
size_t phx_odeint_backprop_workspace_bytes(int N, int H, int B, int T, long long grid_steps);
int phx_odeint_backprop_backward(const phx_params *p, const double *t, int B, int T, const phx_solve_opts *opts,
                                 const float *y_saved, const float *grad_y, float *adj_y0, const phx_grads *grads,
                                 int *status, int *nfe, int *nsteps, void *workspace, size_t workspace_bytes,
                                 void *stream, double step_size, long long grid_steps);
int phx_debug_backprop_kernel_m(int N, int H, int B, int T, int method);
int phx_debug_backprop_launches(int N, int H, int B, int T, int method);
int phx_debug_backprop_plan(int cus, int N, int H, int B, int T, int method, int *plan);

/* prior_grad = X[K,N] @ P[N,N] with the prior matrix P in CSC form
 * (colptr [N+1], rowidx/vals [nnz], rows ascending inside a column).  Replaces the reference's dense
 * `torch.matmul(batch_for_prior, prior_mat)` (train_insilico.py:207-211) and the 0.5 GB dense matrix that
 * `read_prior_matrix(..., sparse=True)` materialises (train_insilico.py:64-73).  out [K,N] is overwritten. */
int phx_prior_targets(const int *colptr, const int *rowidx, const float *vals, const float *X, float *out,
                      int K, int N, void *stream);
/* The same product with P in sliced-ELL form (the fast path; phoenix_amd.prior builds it once per prior matrix):
 * columns in slices of 64; width[s] = longest column of slice s; entry i of column 64 s + l at sptr[s] + i*64 + l in
 * ridx / vals (rows ascending inside a column, padding row 0 / value 0).  X rows are staged in LDS, so N*4 bytes must
 * fit it (PHX_ERR_BAD_ARG otherwise: use phx_prior_targets). */
int phx_prior_targets_sell(const long long *sptr, const int *width, const int *ridx, const float *vals, const float *X,
                           float *out, int K, int N, void *stream);

/* Fused head of the prior branch of training_step (train_insilico.py:134-135):
 *   loss[0] = mean((prior_only_forward(X) - target)^2)  over B*N elements   (device float)
 *   cot[B,N] = d loss / d prior_only_forward(X) = 2 (pred - target) / (B N)
 * without materialising the prediction; `cot` is what phx_rhs_vjp(prior_only = 1) takes for the backward.
 * Workspace: phx_workspace_bytes(PHX_OP_RHS_FORWARD, ...) for B >= 1024 rows; PHX_ERR_BAD_ARG when the batch chain
 * cannot be planned (the caller then evaluates the unfused formula).                                              */
int phx_prior_mse(const phx_params *p, const float *X, const float *target, int B, float *cot, float *loss,
                  void *workspace, size_t workspace_bytes, void *stream);

/* The same step with the hidden rows kept for the backward (ABI 5; what is kept changed in ABI 7).  The forward chain of
 * phx_prior_mse reduces the hidden rows z = [Ws a(X) + bs ; exp(Wp l(X) + bp)] of every row of X anyway, and its last
 * kernel holds the loss cotangent in registers.  phx_prior_mse_save also contracts that cotangent with the rows of Wa
 * there and writes the four hidden sections  du | dv | z_u | z_p  of every row ([4][16 HT][16 ceil(B / 16)] floats, the
 * operand layout of the gradient contraction) to `z_save` (phx_prior_z_bytes(N, H, B) bytes, device, caller-owned; 0 =
 * this shape has no such path: H > 128 or the batch chain cannot be planned).  phx_prior_vjp_saved then computes the
 * parameter gradients of sum(cot * prior_only_forward(X)) -- what phx_rhs_vjp(prior_only = 1, vjp_y = NULL) computes --
 * with the contraction kernel alone: `cot` must be the cotangent phx_prior_mse_save wrote (the caller scales the
 * gradients by d loss afterwards; the saved sections are those of d loss = 1).  Same workspaces as phx_prior_mse /
 * phx_rhs_vjp.  Replaces nothing new in the reference: it is train_insilico.py:134-138 again, with autograd's saved
 * activations made explicit.                                                                                          */
size_t phx_prior_z_bytes(int N, int H, int B);
int phx_prior_mse_save(const phx_params *p, const float *X, const float *target, int B, float *cot, float *loss,
                       float *z_save, void *workspace, size_t workspace_bytes, void *stream);
int phx_prior_vjp_saved(const phx_params *p, const float *X, const float *cot, const float *z_saved,
                        const phx_grads *grads, int B, void *workspace, size_t workspace_bytes, void *stream);

/* the ground-truth Hill-kinetics simulator behind the reference's in-silico data
 * (GraphGRN_core.R:425-486 emits one rate expression per gene -- ode_system_functions_*.csv -- and
 * SimulationGRN_core_init_var.R:218-247 integrates them per sample).  The caller compiles the expressions to
 * postfix programs: code [L][2] = (op, arg) with op 0 PUSHC consts[arg], 1 PUSHX x[arg], 2 ADD, 3 SUB, 4 MUL,
 * 5 DIV, 6 NEG, 7 FACT with consts[arg..arg+2] = (B, K_n, n) of fAct (GraphGRN_core.R:431-436); off/len [N] give each
 * gene's slice (len 0 = "input gene", rate 0).  phx_hill_rhs: out[B,N] = rates at x[B,N].  phx_hill_simulate:
 * out[T,B,N] = states at times[T] (out[0] = x0), classical RK4 with equal sub-steps <= dt_max per interval.       */
int phx_hill_rhs(const int *code, const int *off, const int *len, const float *consts, const float *x,
                 float *out, int B, int N, void *stream);
int phx_hill_simulate(const int *code, const int *off, const int *len, const float *consts, const float *x0,
                      const double *times, int T, double dt_max, float *out, int B, int N, void *stream);

/* The true Jacobian of those rate expressions, the simulator's side of the reference's Jacobian comparators (SURVEY.md row
 * 21: dynamo_extract_matrix.py, helper_true_velo.py).  The programs are those of phx_hill_rhs; the sparse pattern comes in
 * CSR form by target: eptr [N + 1] (eptr[0] = 0, eptr[N] = E, not decreasing) and ereg [E], the regulators of target j in
 * ereg[eptr[j] .. eptr[j + 1]) (the caller lists the distinct PUSHX genes of program j; the call trusts eptr and only
 * compares ereg).  With J[b, e] = d rate_target(e) / d x_ereg[e] at x[b], x [B, N]:
 *     mode 0   out [B, E] = J             mode 1   out [E] = mean over b of J[b, e]        mode 2   out [E] = mean of |J[b, e]|
 * One thread per entry interprets the target's program forward-mode on (value, derivative) pairs in fp32: the value half
 * is phx_hill_rhs's, operation by operation; PUSHC has derivative 0, PUSHX g has (g == ereg[e]), ADD / SUB / NEG are linear,
 * MUL gives l' r + l r', DIV with q = l / r gives (l' - q r') / r, FACT(B, K_n, n) on (tf, tf') gives
 * B K_n n tf^(n-1) / (K_n + tf^n)^2 tf' for tf > 0 and 0 for tf <= 0, where phx_hill_rhs continues fAct by 0.  An ereg[e]
 * that program never pushes gives exactly +0.  Modes 1 and 2 sum in fp64 -- the rows in min(1024, ceil(B / 32)) contiguous
 * chunks, ascending within a chunk, then the chunks in order -- divide by B and round once to fp32: the order depends on B
 * alone, nothing is atomic, two calls agree bit for bit.  Rows and entries are strided over capped grid dimensions: B, N
 * and E are bounded by their types only, and no array is sized by a gene's number of regulators.
 * PHX_ERR_BAD_ARG before any device call: a null code / off / len / consts / eptr / ereg / x / out, B < 1, N < 1, E < 0, a
 * mode outside 0 .. 2.  E == 0: PHX_OK, nothing is launched.  PHX_ERR_WORKSPACE when workspace is null or workspace_bytes <
 * phx_hill_jacobian_workspace_bytes(B, N, E, mode): the chunk sums, [chunks][E] doubles, and 0 where none are needed (mode
 * 0, B <= 32, or arguments the call refuses).  Nothing allocates or synchronises. */
size_t phx_hill_jacobian_workspace_bytes(int B, int N, long long E, int mode);
int phx_hill_jacobian(const int *code, const int *off, const int *len, const float *consts, const long long *eptr,
                      const int *ereg, const float *x, int B, int N, long long E, int mode, float *out, void *workspace,
                      size_t workspace_bytes, void *stream);

/* Knockout screens of that simulator (additive, ABI 7): the truth a model's knockout screen (phx_odeint_clamped +
 * phx_knockout_effects) is scored against.  K calls of B rows all start from the SAME x0 [B, N], which is read once per call
 * and not replicated; call k integrates the system with x[:, genes_host[k]] HELD at values_host[k] -- the column starts at
 * the level and its rate is 0 in every stage, so it keeps the level bit for bit; genes_host[k] == -1 is the unperturbed
 * call.  out [T, K * B, N]: row k * B + b of every time slice belongs to call k (the sol layout of phx_knockout_effects,
 * which scores the block unchanged); out[0] is x0 with the clamped column replaced.  The integrator is phx_hill_simulate's:
 * classical RK4, nsub = max(1, ceil(|span| / dt_max)) equal sub-steps per interval, h = (float)(span / nsub), fp32 state in
 * LDS, fAct continued by 0 at TF <= 0; times [T] (DEVICE, double) may increase or decrease.
 * One workgroup integrates a group of up to KPT calls of one sample: a thread walks its gene's program once per stage and
 * applies every instruction to the KPT operand stacks.  A slot's arithmetic does not depend on the other slots, and a slot
 * without a call integrates the unperturbed system and stores nothing (no remainder path): the bits of call k are the same
 * whether it runs alone, first or last in a group, beside a duplicate of itself or in a remainder group, so a gene the
 * clamped gene cannot reach has a shift of exactly 0 against the -1 call.  KPT = 2 up to 4 096 genes and 1 above: 2 measured
 * fastest of 1, 2, 4, 8 on the shipped 350-gene network (profiles/hill_knockouts.json), and KPT x (genes per thread) <= 8.
 * phx_debug_hill_knockouts_kpt(N): the KPT a call uses at N genes (0: N refused); PHX_HILLKO_KPT = 1 | 2 | 4 | 8 in the
 * environment asks for another one, cut to that budget (tools/bench_hill_knockouts.py times them).
 * genes_host / values_host [K] are HOST arrays: checked before any device call and handed to the kernel as launch
 * arguments, 256 calls per launch.  Groups and rows are strided over capped grid dimensions: neither K nor B is bounded by
 * one.  Nothing allocates, copies from pageable memory or synchronises.
 * PHX_ERR_BAD_ARG with nothing launched: a null pointer, B / N / K / T < 1, dt_max not > 0, N > 8 192, a gene outside
 * -1 .. N - 1, a level that is not finite, K * B beyond int. */
int phx_hill_knockouts(const int *code, const int *off, const int *len, const float *consts, const float *x0,
                       const double *times, int T, double dt_max, const int *genes_host, const float *values_host, int K,
                       float *out, int B, int N, void *stream);
int phx_debug_hill_knockouts_kpt(int N);

/* phx_hill_knockouts with a held SET per call (additive, ABI 7): the truth of a combination screen (phx_odeint_clamped_sets
 * + phx_knockout_epistasis).  genes_host / values_host are HOST arrays [K, width], row-major, 1 <= width <=
 * PHX_HILL_HOLD_MAX: call k starts from x0 with every gene of row k set to that entry's level, and the rate of each of them
 * is 0 in every stage of every sub-step.  -1 entries pad a shorter set and their level is not looked at; a row of -1 alone
 * is the unperturbed call.  Everything else is phx_hill_knockouts: the out [T, K * B, N] layout, the integrator, the
 * interpreter, the calls per workgroup and genes per thread, no remainder path, strided grids.  The width of a slot's row
 * is a template parameter of the same kernel, instantiated at 1 (phx_hill_knockouts itself), 2 and 4 -- a width of 3 runs
 * at 4 -- and the one difference is the clamp test, "the gene is in the slot's row".  A (gene, slot) that is not held is
 * computed without a look at the row: the bits of a call do not depend on the width it runs at, on the order of its row
 * or on the calls beside it, so a 1-entry row equals the phx_hill_knockouts call, and a gene that one held gene of a pair
 * cannot reach has the bits it has in the other gene's single call -- the second difference of a pair screen is exactly 0
 * at every target that is not a common descendant of both.  The launch arguments stay at 2 KiB: 256 / 128 / 64 calls per
 * launch at the instantiated widths 1 / 2 / 4.  Nothing allocates, copies from pageable memory or synchronises.
 * PHX_ERR_BAD_ARG with nothing launched: everything phx_hill_knockouts refuses, width < 1 or > PHX_HILL_HOLD_MAX, an entry
 * outside -1 .. N - 1, a level that is not finite on an entry that is not -1, a gene twice in one row (two levels would be
 * ambiguous). */
#define PHX_HILL_HOLD_MAX 4
int phx_hill_knockout_sets(const int *code, const int *off, const int *len, const float *consts, const float *x0,
                           const double *times, int T, double dt_max, const int *genes_host, const float *values_host,
                           int width, int K, float *out, int B, int N, void *stream);

/* The steady states (attractors) of the simulator by implicit relaxation (additive, ABI 7; DESIGN.md section 8p,
 * phx_hillss.hip): per row of x0 [R, N] the iteration (sigma I - J(x)) delta = f(x), sigma = 1 / tau (0 for tau = inf:
 * Newton), x <- x + delta under the control of phoenix_amd.steady_states -- rho = max |f| over the moving genes; done at
 * rho <= tol (compared in float); a step is accepted iff the new rho' is finite and <= 2 rho, then tau <- tau min(10, max(2,
 * rho / rho')), else x stays and tau <- tau / 4.  f are the rates of phx_hill_rhs, J their Jacobian on the pattern (eptr,
 * ereg, E) of phx_hill_jacobian, by the same interpreter rules.  The schedule, device int32: order [N] lists the genes by
 * strongly connected component of the pattern without its diagonal, the components by level (1 + the highest level of a
 * component that regulates it); comp_ptr [n_comp + 1] cuts order into components, level_ptr [n_level + 1] the components into
 * levels; largest is the size of the largest component.  A step is a forward substitution over the levels: a one-gene
 * component is delta_j = (f_j + sum_{k != j} J_jk delta_k) / (sigma - J_jj) in float, the row's entries ascending; a larger one
 * solves its block in double by LU with partial pivoting.  A gene with an empty program or moving[r, n] == 0 (moving: uint8
 * [R, N], NULL: every gene with a program moves) has f = 0 and delta = 0 and keeps its x0 bits.
 * One launch, one workgroup per row, no atomics; the bits of a row do not depend on R or on the other rows.
 * Outputs: x [R, N]; residual [R] = rho at x; iterations [R] = the steps tried; status [R] = 0 converged, 1 max_iter reached,
 * 2 a zero or non-finite pivot or divisor (x is the last accepted state); tau [R].
 * phx_hill_steady_lds_bytes: the LDS of a workgroup, 0 for a system the call refuses (largest > PHX_HILL_SCC_MAX or more
 * than 64 KiB: (largest^2 + largest) doubles for largest > 1, and 5 N + E + 6 words).
 * PHX_ERR_BAD_ARG before any launch: such a system, a null pointer other than moving, R < 1, N < 1, E < 0, max_iter < 0,
 * n_comp outside 1 .. N, n_level outside 1 .. n_comp, tol not finite or < 0, tau0 not > 0. */
#define PHX_HILL_SCC_MAX 64
size_t phx_hill_steady_lds_bytes(int N, long long E, int largest);
int phx_hill_steady(const int *code, const int *off, const int *len, const float *consts, const long long *eptr,
                    const int *ereg, long long E, const int *order, const int *comp_ptr, int n_comp, const int *level_ptr,
                    int n_level, int largest, const float *x0, const unsigned char *moving, int R, int N, double tol,
                    int max_iter, double tau0, float *x, float *residual, int *iterations, int *status, float *tau,
                    void *stream);

/* the scoring tail of the gene-influence scan (find_gene_influences.py:64-77) on the solver's
 * own output.  sol [T, 2 * pairs * B, N] is the block phx_odeint wrote for 2 * pairs calls of B rows (opts->calls): call
 * 2j is the unperturbed solve of pair j, call 2j + 1 the perturbed one; genes_host [pairs] (HOST) names the perturbed
 * gene of every pair.  With
 *     s[j, n]       = sum over tau = 1 .. T-1, b < B of | sol[tau, 2jB + b, n] - sol[tau, (2j+1)B + b, n] |
 *     targets[j, n] = s[j, n] / ((T-1) B)                             mean |difference| of target gene n  (may be NULL)
 *     scores[j]     = (sum over n != genes[j] of s[j, n]) / ((T-1) B (N-1))                        (:74-75)
 * sol is read once (its tau = 0 slab not at all), every sum runs in an order fixed by the shape (no atomics: two calls
 * on the same block agree bit for bit, with or without targets), column genes[j] is left out of the score by index and
 * reported in targets as computed.  Non-finite inputs propagate (a NaN trajectory gives a NaN score).
 * PHX_ERR_BAD_ARG before any device call: null sol / scores / genes_host, T < 2, pairs < 1 (or > 65535), B < 1, N < 2,
 * a gene outside [0, N); PHX_ERR_WORKSPACE when workspace_bytes < phx_influence_workspace_bytes(T, pairs, B, N) (0 for a
 * shape the call refuses): s lives there when targets is NULL. */
size_t phx_influence_workspace_bytes(int T, int pairs, int B, int N);
int phx_influence_scores(const float *sol, int T, int pairs, int B, int N, const int *genes_host, float *scores,
                         float *targets, void *workspace, size_t workspace_bytes, void *stream);

/* The scoring pass of a knockout screen: K clamped solves (phx_odeint_clamped) against ONE unperturbed solve.
 * base [T, B, N] is the output block of the baseline, sol [T, K * B, N] that of K calls of B rows started from the same
 * states with gene genes_host[k] (HOST, [K]) set to its clamped level.  With d = sol[tau, kB + b, n] - base[tau, b, n]
 * over tau = 1 .. T-1 and b < B:
 *     shift[k, n]     = mean of d          signed: does target n go up or down            (may be NULL)
 *     magnitude[k, n] = mean of |d|                                                       (may be NULL)
 *     scores[k]       = mean of magnitude[k, n] over n != genes[k]     (find_gene_influences.py:74-75, one shared baseline)
 * sol is read once (its tau = 0 slab not at all); no pair layout, no replicated baseline.  Every sum runs in an order
 * fixed by the shape (no atomics): two calls agree bit for bit, with or without the optional outputs.  Column genes[k] is
 * left out of the score by index and reported in shift / magnitude as computed.  Non-finite inputs propagate.
 * PHX_ERR_BAD_ARG before any device call: null base / sol / scores / genes_host, T < 2, K < 1 (or > 65535), B < 1, N < 2,
 * a gene outside [0, N); PHX_ERR_WORKSPACE when workspace is null or workspace_bytes <
 * phx_knockout_effects_workspace_bytes(T, K, B, N) (0 for a shape the call refuses): the sums live there. */
size_t phx_knockout_effects_workspace_bytes(int T, int K, int B, int N);
int phx_knockout_effects(const float *base, const float *sol, int T, int K, int B, int N, const int *genes_host,
                         float *scores, float *shift, float *magnitude, void *workspace, size_t workspace_bytes,
                         void *stream);

/* The scoring pass of a PAIR screen: K calls that hold two genes each (phx_odeint_clamped_sets) against the unperturbed
 * solve and the two single-gene calls of every pair.  base [T, B, N]; singles [T, G * B, N]: G single-gene calls, the sol
 * layout of phx_knockout_effects, single g holding gene genes_host[g] (HOST, [G]); sol [T, K * B, N]: K pair calls, pair k
 * holding the genes of singles ia_host[k] and ib_host[k] (HOST, [K], indices into the G singles).  All differences are
 * float32, over tau = 1 .. T-1 and b < B, with d_x = x - base and e = d_ab - (d_a + d_b) (symmetric in a and b: swapping
 * the pair changes no bit).  Every matrix is [K, N] and may be NULL:
 *     shift[k, n]                 = mean of d_ab
 *     magnitude[k, n]             = mean of |d_ab|
 *     interaction[k, n]           = mean of e        the joint effect beyond the sum of the single ones (epistasis)
 *     interaction_magnitude[k, n] = mean of |e|
 *     scores[k]                   = mean of magnitude[k, n] over n not in {a, b}                (required)
 *     interaction_scores[k]       = mean of interaction_magnitude[k, n] over n not in {a, b}    (required)
 * The two held columns are skipped by index, not subtracted from a total (on column a, e is -d_b[a], no interaction, and
 * it dominates the row), and reported in the matrices as computed.  sol and the singles are read once (their tau = 0 slabs
 * not at all); every sum runs in an order fixed by (T, B, N) alone (no atomics): two calls agree bit for bit, with or
 * without the optional outputs, and however the K pairs are split over calls.  Non-finite inputs propagate.
 * PHX_ERR_BAD_ARG before any device call: null base / singles / sol / ia_host / ib_host / genes_host / scores /
 * interaction_scores, T < 2, K < 1 (or > 65535), G < 2, B < 1, N < 3, an index outside [0, G), ia[k] == ib[k], a gene
 * outside [0, N); PHX_ERR_WORKSPACE when workspace is null or workspace_bytes <
 * phx_knockout_epistasis_workspace_bytes(T, K, G, B, N) (0 for a shape the call refuses): the sums live there. */
size_t phx_knockout_epistasis_workspace_bytes(int T, int K, int G, int B, int N);
int phx_knockout_epistasis(const float *base, const float *singles, const float *sol, int T, int K, int G, int B, int N,
                           const int *ia_host, const int *ib_host, const int *genes_host, float *scores,
                           float *interaction_scores, float *shift, float *magnitude, float *interaction,
                           float *interaction_magnitude, void *workspace, size_t workspace_bytes, void *stream);

/* The explainability matrices of a trained model, regulator i -> target j (the orientation of effects_mat and of the
 * gene-influence matrix), from the engine layout as it is.  With s = y - 0.5 and r = relu(g):
 *     S[i,j]   = sum_h Ws[h,i] WaT[h,j]                                          (state independent)
 *     Q_b[i,j] = sum_h p[b,h] Wp[h,i] WaT[H+h,j]                                 p[b,:] = exp(Wp log1p(softsign(s_b)) + bp)
 *     J_b[i,j] = d f_j / d y_i (y_b) = r_j ( a'(y_bi) S[i,j] + l'(y_bi) Q_b[i,j] - delta_ij )       (odenet.py:85-91)
 *     a' = 1 / (1 + |s|)^2          l' = 1 / (1 + |s|) for s < 0,   1 / ((1 + s)(1 + 2 s)) for s >= 0
 *     effects[i,j] = r_j ( S[i,j] + sum_h Wp[h,i] WaT[H+h,j] )                   (extract_model_matrix_PHOENIX.py:46-58;
 *                                                                                 J with a' = l' = p = 1 and no delta)
 * PHX_EFFECTS writes `effects` (y, ph and B are ignored), PHX_JAC_MEAN (1/B) sum_b J_b, PHX_JAC_MEAN_ABS (1/B) sum_b |J_b|
 * over the states y [B, N].  ph [B, H] is the caller's product-branch hidden vector p[b,:] of those states; a' and l' are
 * computed from y by the closed forms.  out [row1 - row0, N] (row-major) receives regulator rows row0 .. row1 - 1 only, so
 * that a caller can walk a genome-scale matrix in chunks; delta belongs to global row i = column j whatever row0 is.
 * One launch (phx_effects.hip): every 64 x 64 tile stays in MFMA accumulators over the hidden rows and over all B states,
 * out is written exactly once and no N x N temporary is read or written.  Every entry is summed by one wave in an order
 * fixed by (N, H, B, mode, i, j): no atomics, and its bits do not depend on the row range.  relu(g_j) = 0 gives exact
 * zeros in column j; non-finite inputs propagate.  Of `p` the call reads Ws, Wp, WaT and g.
 * PHX_ERR_BAD_ARG before any device call: null p / out / Ws / Wp / WaT / g, N < 2, H < 1, H > 256, row0 < 0, row1 > N,
 * row0 >= row1, an unknown mode, a Jacobian mode with null y or ph or B < 1.  PHX_ERR_WORKSPACE when workspace_bytes <
 * phx_effects_workspace_bytes(N, H, B, mode) (0 when none is needed or the shape is refused; today no shape needs any). */
enum phx_effects_mode { PHX_EFFECTS = 0, PHX_JAC_MEAN = 1, PHX_JAC_MEAN_ABS = 2 };
size_t phx_effects_workspace_bytes(int N, int H, int B, int mode);
int phx_effects_matrix(const phx_params *p, int mode, const float *y, const float *ph, int B, int row0, int row1,
                       float *out, void *workspace, size_t workspace_bytes, void *stream);

/* The strongest regulator -> target edges of those matrices without the matrices: M = what phx_effects_matrix writes for
 * (mode, y, ph, B), entry M[i,j] eligible when it is finite and non-zero, i != j (or PHX_EDGES_DIAGONAL is set) and, with
 * PHX_EDGES_ORIENT, |M[i,j]| > |M[j,i]| strictly (make_mask of extract_model_matrix_PHOENIX.py:29-37: of every gene pair the
 * stronger direction only; the diagonal is then never eligible, an equally strong pair loses both directions, a NaN partner
 * loses the comparison).  Magnitudes are compared as m = bits & 0x7fffffff.  phx_edges.hip runs the tile engine of
 * phx_effects_matrix with a selection epilogue in place of the store (with ORIENT a workgroup forms tiles (I, J) and (J, I)
 * and transposes one through LDS): every reported value has the bits phx_effects_matrix writes for that entry, and no
 * N x N buffer is read or written.  A selection is a sequence of passes, each ONE launch that recomputes every tile (in the
 * Jacobian modes each pass therefore repeats the loop over the B states); the caller reads the small results between them:
 *   PHX_EDGES_COUNT  workspace: unsigned hist[4096] (zeroed by the call, then summed with integer atomics: exact and
 *                    independent of arrival order).  level 0: hist[m >> 19] over all eligible entries; level 1:
 *                    hist[(m >> 7) & 4095] over the eligible entries with (m >> 19) == prefix.  From the top, the bin where
 *                    the running sum reaches K bounds the K strongest edges; the sum down to a bin sizes the next pass.
 *   PHX_EDGES_EMIT   every eligible entry with |M[i,j]| >= tau is appended: keys[n] = (0x7fffffff - m) << 32 | (i N + j),
 *                    values[n] = M[i,j], in no particular order; workspace: unsigned count at byte 16384 (zeroed by the
 *                    call) = how many entries qualified.  Entries beyond `capacity` are counted and not written, so
 *                    count > capacity tells a too-small buffer and by how much.  Sorting the keys ascending orders the
 *                    edges by magnitude descending, then i, then j: the sorted list is bitwise reproducible.
 * keys, values and capacity are ignored by COUNT; level and prefix by EMIT, tau by COUNT.  Nothing allocates or synchronises.
 * PHX_ERR_BAD_ARG before any device call: null p / Ws / Wp / WaT / g, N < 2, N > 65535 (i N + j is 32 bits of the key),
 * H < 1, H > 256, an unknown mode, a Jacobian mode with null y or ph or B < 1, unknown flags, an unknown pass, a level
 * other than 0 and 1, a level-1 prefix >= 0xff0 (not finite), EMIT with null keys or values, capacity < 1, or tau not
 * positive and finite.  PHX_ERR_WORKSPACE when workspace is null or workspace_bytes <
 * phx_effects_edges_workspace_bytes(N, H, B, mode) (16448 for a served shape, 0 for one the call refuses). */
enum phx_edges_flags { PHX_EDGES_ORIENT = 1, PHX_EDGES_DIAGONAL = 2 };
enum phx_edges_pass { PHX_EDGES_COUNT = 0, PHX_EDGES_EMIT = 1 };
size_t phx_effects_edges_workspace_bytes(int N, int H, int B, int mode);
int phx_effects_edges(const phx_params *p, int mode, const float *y, const float *ph, int B, int flags, int pass, int level,
                      unsigned prefix, float tau, long long *keys, float *values, unsigned capacity, void *workspace,
                      size_t workspace_bytes, void *stream);

/* Scoring those matrices against a known network (the network-recovery AUROC of the PHOENIX paper; the reference's only
 * scorer, COMPUTE_GRN_AUROC of GRN_rnaode.py:10-22, walks a Python list of all N^2 edges) without the matrices: the two
 * device passes of phx_netscore.hip, each ONE launch of the tile engine of phx_effects_matrix that recomputes every tile.
 * M = what phx_effects_matrix writes for (mode, y, ph, B).  The SCORED matrix is M itself or, with PHX_EDGES_ORIENT,
 * make_mask of M (extract_model_matrix_PHOENIX.py:29-37): an entry keeps its value only when |M[i,j]| > |M[j,i]| as floats,
 * strictly (a NaN on either side fails the comparison); every other entry and the whole diagonal are +0.  The score of an
 * entry is its magnitude bits m = bits & 0x7fffffff.  Scored entries: all i != j inside N, and the diagonal too with
 * PHX_EDGES_DIAGONAL (RANK only; GATHER answers whatever it is asked).  Zeros are scored like every other value.
 *   phx_effects_gather       values[n] = the scored matrix's entry keys[n] = i N + j, n < n_keys (duplicates allowed), with
 *                            the bits of that entry.  The keys are grouped by 64 x 64 tile: with T = ceil(N / 64) the keys of
 *                            tile t = (i / 64) T + j / 64 are keys[tile_offsets[t] .. tile_offsets[t + 1]), tile_offsets
 *                            [T T + 1] ascending from 0 to n_keys (offsets are clamped to n_keys; a key that does not lie in
 *                            the tile of its segment receives a NaN).  Workgroups whose segments are empty form no tile.
 *   phx_effects_rank_counts  u [m] = distinct magnitude bits, ascending (the caller's positives).  counts [2 m + 1] (zeroed by
 *                            the call): every scored entry of magnitude x is counted once, in counts[2 lb + 1] when
 *                            u[lb] == x and in counts[2 lb] otherwise, lb = #{k : u[k] < x}; so counts[2 k + 1] entries tie
 *                            with u[k] and counts[2 k] lie strictly between u[k - 1] and u[k].  A non-finite scored entry is
 *                            counted in the unsigned at byte 0 of the workspace (zeroed by the call) and in no bucket.
 *                            Integer atomics only: the counts are exact and independent of arrival order; the two lowest
 *                            and two highest buckets leave each workgroup as one atomic.
 * Nothing allocates or synchronises.  PHX_ERR_BAD_ARG before any device call: null p / Ws / Wp / WaT / g, N < 2, N > 65535
 * (a key is 32 bits and a count fits 32), H < 1, H > 256, an unknown mode, a Jacobian mode with null y or ph or B < 1,
 * unknown flags; gather: null keys / tile_offsets / values, n_keys < 1; rank: null u / counts, m < 1, m > 2^31 - 1.
 * PHX_ERR_WORKSPACE (rank) when workspace is null or workspace_bytes < phx_effects_rank_workspace_bytes(N, H, B, mode) (64
 * for a served shape, 0 for one the calls refuse). */
size_t phx_effects_rank_workspace_bytes(int N, int H, int B, int mode);
int phx_effects_gather(const phx_params *p, int mode, const float *y, const float *ph, int B, int flags, const unsigned *keys,
                       const unsigned *tile_offsets, unsigned n_keys, float *values, void *stream);
int phx_effects_rank_counts(const phx_params *p, int mode, const float *y, const float *ph, int B, int flags, const unsigned *u,
                            unsigned m, unsigned *counts, void *workspace, size_t workspace_bytes, void *stream);

/* Every gene's k strongest regulators or targets in those matrices, with its degree and weighted degree, without the
 * matrices: M = what phx_effects_matrix writes for (mode, y, ph, B).  Entry M[i,j] (regulator i -> target j) is eligible
 * under the rules of phx_effects_edges (finite and non-zero on m = bits & 0x7fffffff; i != j unless PHX_EDGES_DIAGONAL; with
 * PHX_EDGES_ORIENT |M[i,j]| > |M[j,i]| strictly, never the diagonal, a NaN partner loses) and, in addition, when
 * regulator_ok[i] != 0, target_ok[j] != 0 (unsigned char [N] each; null: every gene) and |M[i,j]| >= tau (tau = +0: no
 * threshold).  axis = PHX_NEIGHBORS_OF_TARGET: line n is column n, the regulators of target n; PHX_NEIGHBORS_OF_REGULATOR:
 * line n is row n, the targets of regulator n.  For every line n < N:
 *   gene  [N, k], value [N, k]   the k strongest eligible entries of the line: the OTHER gene's index and the entry with the
 *                                bits phx_effects_matrix writes, by magnitude descending, then by that index ascending;
 *                                a line with fewer than k eligible entries is padded with gene = -1, value = +0.
 *   count [N]                    the eligible entries of the line (the in- or out-degree at tau): an exact integer.
 *   strength [N]                 the float sum of their magnitudes (the weighted degree).
 * phx_neighbors.hip: a workgroup owns 64 lines and streams the 64 x 64 tiles of the other dimension through the tile engine
 * of phx_effects_matrix (with ORIENT the partner tile too), selecting in the epilogue; the streamed dimension is cut into S
 * segments, S a function of N alone (PHX_NEIGHBORS_SEGMENTS=<n> in the environment, read per call, forces n; S <= 8 and
 * <= ceil(N / 64) always), whose lists, counts and sums a second small kernel merges in segment order.  No atomics: the
 * lists are sets selected by a total order, every float sum has an order fixed by (N, S), so all four results are bitwise
 * reproducible.  A line tile or a streamed tile without a candidate is not formed.  Nothing allocates or synchronises.
 * PHX_ERR_BAD_ARG before any device call: null p / Ws / Wp / WaT / g, N < 2, N > 65535 (a gene index is 16 bits of the key),
 * H < 1, H > 256, an unknown mode, a Jacobian mode with null y or ph or B < 1, unknown flags, an unknown axis, k < 1, k > 64,
 * tau negative, not finite or -0, a null result.  PHX_ERR_WORKSPACE when workspace is null or workspace_bytes <
 * phx_effects_neighbors_workspace_bytes(N, H, B, mode, axis, k) (0 for arguments the call refuses; it reads the same
 * environment switch). */
enum phx_neighbors_axis { PHX_NEIGHBORS_OF_REGULATOR = 0, PHX_NEIGHBORS_OF_TARGET = 1 };
size_t phx_effects_neighbors_workspace_bytes(int N, int H, int B, int mode, int axis, int k);
int phx_effects_neighbors(const phx_params *p, int mode, const float *y, const float *ph, int B, int flags, int axis, int k,
                          float tau, const unsigned char *regulator_ok, const unsigned char *target_ok, int *gene, float *value,
                          unsigned *count, float *strength, void *workspace, size_t workspace_bytes, void *stream);

/* Products of a block of vectors with those matrices, taken after the same element-wise rules and without the matrices: M =
 * what phx_effects_matrix writes for (mode, y, ph, B), entry M[i,j] eligible exactly as for phx_effects_neighbors (flags,
 * regulator_ok, target_ok, tau and axis as there).  V and out are [N, R] row-major float, 1 <= R <= 32 per call:
 *   PHX_NEIGHBORS_OF_TARGET      out[n, r] = sum over the eligible i of w(M[i,n]) V[i, r]    (M^T V: regulator -> target)
 *   PHX_NEIGHBORS_OF_REGULATOR   out[n, r] = sum over the eligible j of w(M[n,j]) V[j, r]    (M V)
 * with w the entry (PHX_APPLY_VALUE), its magnitude (PHX_APPLY_ABS) or 1.0f (PHX_APPLY_UNIT).  An ineligible entry
 * contributes nothing -- it is skipped, not multiplied by zero -- so a non-finite entry of M never reaches out, a non-finite
 * V[g, r] reaches only the lines with an eligible entry at gene g, and a line without an eligible entry is exactly +0.  Rows
 * of V at or beyond N are never read.
 * phx_apply.hip: the line-tile x segment grid of phx_neighbors.hip (S from the same rule and the same switch
 * PHX_NEIGHBORS_SEGMENTS); lane l of each of a workgroup's four waves owns line l, wave q takes entries 16 q .. 16 q + 15 of
 * every streamed 64 x 64 tile, whose 64 x R slice of V lies in LDS.  out[n, r] is a float sum in an order fixed by (N, S)
 * alone: per (line, q) fmaf(w, V, acc) over the segment's streamed tiles ascending and the 16 entries of each ascending,
 * then ((a0 + a1) + a2) + a3 over q, then the S partials in segment order (a second small kernel).  The bits of column r
 * depend neither on R nor on where in the block the column stands.  No atomics, plain global stores; a line tile or a
 * streamed tile without a candidate is not formed.  Nothing allocates or synchronises.
 * PHX_ERR_BAD_ARG before any device call: everything phx_effects_neighbors refuses of (p, mode, y, ph, B, flags, axis, tau),
 * N > 65535 included, an unknown weight, R < 1, R > 32, a null V or out.  PHX_ERR_WORKSPACE when workspace is null or
 * workspace_bytes < phx_effects_apply_workspace_bytes(N, H, B, mode, axis, R) (the S partial blocks; 0 for arguments the
 * call refuses; it reads the same environment switch). */
enum phx_apply_weight { PHX_APPLY_VALUE = 0, PHX_APPLY_ABS = 1, PHX_APPLY_UNIT = 2 };
size_t phx_effects_apply_workspace_bytes(int N, int H, int B, int mode, int axis, int R);
int phx_effects_apply(const phx_params *p, int mode, const float *y, const float *ph, int B, int flags, int axis, int weight,
                      float tau, const unsigned char *regulator_ok, const unsigned char *target_ok, const float *V, int R,
                      float *out, void *workspace, size_t workspace_bytes, void *stream);

/* Pathway permutation tests on one score per gene (the reference's create_permutation_test_files_aws.R, whose 500 draws per
 * pathway this call replaces).  scores [N] float; the P pathways in CSR form: ptr [P + 1] (ptr[0] = 0, non-decreasing,
 * ptr[P] = nnz) and idx [nnz], the member genes of pathway p at [ptr[p], ptr[p + 1]), each inside [0, N) and unique within
 * its pathway -- the caller vouches for ptr and idx, they are on the device and are not checked.  Permutation number r in
 * [first, first + n_perm) is defined by (seed, r) alone, in arithmetic modulo 2^64:
 *   c = r << 14 | g                                          for gene g < N <= 16384, r < 2^50
 *   mix(z): z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  return z ^ z >> 31
 *   key[g] = (mix(mix(seed + 0x9E3779B97F4A7C15 * (c + 1))) & ~0x3FFF) | g        (the low 14 bits make keys distinct)
 *   order_r = the genes by ascending key;  permuted_r[g] = scores[order_r[g]];  x_r[p] = sum of permuted_r over pathway p
 * Every pathway sees the same permutation r (the reference draws one per pathway and replicate; each pathway's null
 * distribution is the same either way).  The sums are double, in an order that depends on the pathway's member list alone.
 *   base  [P]   that sum over `scores` themselves, in the same order
 *   count [P]   #{r : base < x_r}, strict as the reference's mean(base_res < all_perm_results)
 *   s1, s2 [P]  sum_r (x_r - base) and sum_r (x_r - base)^2: shifted by base so that the variance does not cancel
 * phx_pathways.hip: min(n_perm, 512) workgroups take the permutations round-robin; one permutation is 8-byte keys sorted
 * in LDS (a bitonic network over the next power of two, 128 KiB at N = 16384) and then the permuted scores in the same LDS;
 * 16 lanes walk a pathway's members, read as 16-bit words; a second kernel adds the workgroups' partials in order.  No
 * atomics: base and count are exact, s1 and s2 are sums whose order is fixed by (first, n_perm) -- never by the device -- so
 * identical calls give identical bits, and a range split by `first` over calls or devices gives the same counts.
 * Nothing allocates or synchronises.  PHX_ERR_BAD_ARG before any device call: N < 1, N > 16384, P < 1, nnz < 0, n_perm < 1,
 * first < 0, first + n_perm > 2^50, a null scores / ptr / result, a null idx with nnz > 0.  PHX_ERR_WORKSPACE when workspace
 * is null or workspace_bytes < phx_pathway_permutations_workspace_bytes(N, P, nnz, n_perm) (0 for arguments the call
 * refuses): the narrowed member list and 24 bytes per workgroup and pathway. */
size_t phx_pathway_permutations_workspace_bytes(int N, int P, long long nnz, long long n_perm);
int phx_pathway_permutations(const float *scores, int N, const long long *ptr, const int *idx, int P, long long nnz,
                             unsigned long long seed, long long first, long long n_perm, double *base, long long *count,
                             double *s1, double *s2, void *workspace, size_t workspace_bytes, void *stream);

/* The reduced Jacobian of the steady-state solve (phoenix_amd.steady_states).  On the genes that move,
 * f(y) = relu(g) (Wa h(y) - y) with h(y) = [Ws a(y) + bs ; exp(Wp l(y) + bp)]; with C(y) = [Ws diag(a'(y)) ;
 * diag(v) Wp diag(l'(y))], v = exp(Wp l(y) + bp), a linearly implicit step of per-gene weights m is delta = m (r + Wa x),
 * (I - S) x = w.  For the B states y [B, N] and weights m [B, N] (float, any values; exact 0 marks a gene that takes no
 * part: its derivative and its residual are not read into any sum) the call writes, all float:
 *   S   [B, 2H, 2H]   S_b = C(y_b) diag(m_b) Wa
 *   w   [B, 2H]       w_b = C(y_b) (m_b r_b), where r [B, N] is given; r and w are both null or both given
 *   hid [B, 2H]       (Ws a(y_b) + bs, exp(Wp l(y_b) + bp)), the hidden vector, over ALL genes
 * phx_steady.hip: one contraction over the genes with the rows of Ws / Wp as A operands and the N x (2H + 2) block
 * [diag(d m) WaT^T | act | d m r] as B operand, v_mfma_f32_16x16x4_f32.  A workgroup owns a 64 x 64 output block of one
 * branch, a segment of the gene axis and four states; 32 genes of its weight rows at a time stay in LDS while it walks the
 * states.  The gene axis is cut into S = min(ceil(N / 32), ceil(256 / blocks(H))) segments, a function of (N, H) alone; a
 * second kernel adds the segments' partial blocks in segment order, adds the bias, takes exp and scales the product rows by
 * v_j.  No atomics.  The bits of a state depend neither on B nor on the other states of the call.  More states than 64 MiB
 * of partial blocks hold are walked in chunks inside the call.  Nothing allocates or synchronises.
 * 1 <= H <= 256, N >= 1, B >= 1.  PHX_ERR_BAD_ARG before any device call: null p / Ws / bs / Wp / bp / WaT / y / m / S / hid,
 * a shape outside those ranges, r without w or w without r.  PHX_ERR_WORKSPACE when workspace is null or workspace_bytes <
 * phx_reduced_jacobian_workspace_bytes(N, H, B) (0 for a shape the call refuses). */
size_t phx_reduced_jacobian_workspace_bytes(int N, int H, int B);
int phx_reduced_jacobian(const phx_params *p, const float *y, const float *m, const float *r, int B, float *S, float *w,
                         float *hid, void *workspace, size_t workspace_bytes, void *stream);
/* The RHS-sized passes and the dense solve of that iteration, each in a sum order fixed by the shape alone, so that a
 * state's bits do not depend on the batch it is solved in.  B <= 65535 for the first two.
 * phx_steady_residual: hid [B, 2H] as above and r [B, N] = Wa hid - y (c ascending per gene).
 * phx_steady_update:   out [B, N] = y + m (r + Wa x) where m != 0, y (to the bit) where m == 0; x [B, 2H].
 * phx_steady_solve:    (I - S_b) x_b = w_b in double, LU with partial pivoting, one workgroup per state; x [B, 2H] float,
 *   info [B] = 0, k + 1 where column k has no finite non-zero pivot, -1 where the solution is not finite as float (x_b = 0 for both).
 *   workspace: phx_steady_solve_workspace_bytes(H, B) = B (2H)^2 doubles.
 * PHX_ERR_BAD_ARG before any device call for a null pointer or a shape outside the ranges, PHX_ERR_WORKSPACE as above. */
int phx_steady_residual(const phx_params *p, const float *y, int B, float *hid, float *r, void *stream);
int phx_steady_update(const phx_params *p, const float *y, const float *m, const float *r, const float *x, int B, float *out,
                      void *stream);
size_t phx_steady_solve_workspace_bytes(int H, int B);
int phx_steady_solve(const float *S, const float *w, int H, int B, float *x, int *info, void *workspace, size_t workspace_bytes,
                     void *stream);

/* The implicit adjoint of that solve (phoenix_amd.steady_states(differentiable=True)).  A steady state
 * satisfies P r(y*) = 0, (I - P) y* = (I - P) y0 with r(y) = Wa h(y) - y and P = diag(m), m = 1 on the genes that move and 0 on
 * the others.  With gy = dL/dy* [B, N], per row:
 *     b = WaT (m gy),   (I - S^T) q = b   (S of phx_reduced_jacobian at y* with this m; phx_steady_solve on its transpose),
 *     u = gy + C^T q,   lam = m u,   dL/dy0 = (1 - m) u
 * and the parameter gradients are sums over the rows: dWa[n, c] = sum lam[b, n] hid[b, c], dWs[j, n] = sum q[b, j] a[b, n],
 * dWp[j, n] = sum q[b, H + j] v[b, j] l[b, n], dbs[j] = sum q[b, j], dbp[j] = sum q[b, H + j] v[b, j], dg = 0 (a fixed point
 * does not depend on the size of a positive multiplier).  phx_steady_adj.hip; all arrays float on the device.
 * phx_steady_adjoint_project: b [B, 2H].  A contraction over the genes, v_mfma_f32_16x16x4_f32, 64 rows x 64 columns per
 *   workgroup; the gene axis is cut into min(ceil(N / 32), 8) segments, a function of N alone, whose partial blocks
 *   (workspace: phx_steady_adjoint_project_workspace_bytes(N, H, B)) a second kernel adds in ascending order.  A gene with
 *   m == 0 is not read into any sum, whatever gy holds there.  A row's bits depend neither on B nor on the other rows.
 * phx_steady_adjoint_back: lam [B, N] and gy0 [B, N] from y, m, gy, q [B, 2H] and hid [B, 2H] (phx_reduced_jacobian's).  One
 *   thread per gene, j ascending, a' and l' recomputed from y.  lam is exactly 0 where m == 0, gy0 exactly 0 where m != 0.
 *   B <= 65535.
 * phx_steady_param_grads: the five products from y, lam, q, hid into `grads`, which is honoured as phx_rhs_vjp honours it
 *   (overwrite, Wa or WaT); grads->g is written 0 under overwrite and left untouched otherwise.  The products are one
 *   [4H] x (N + 1) block (gene N is a column of ones: the bias sums) and the contraction runs over the rows:
 *   v_mfma_f32_16x16x4_f32, a workgroup owns 64 columns x 64 genes and walks its rows 32 at a time, a and l recomputed once
 *   per (row, gene) of a chunk.  The rows are cut into max(1, min(ceil(B / 32) / 2, ceil(512 / blocks))) segments, a function
 *   of (N, H, B) alone; finishing kernels add the segments' partial blocks (workspace:
 *   phx_steady_param_grads_workspace_bytes(N, H, B)) in ascending order and write every output element once.  A row with
 *   lam = 0 and q = 0 contributes exact zeros.
 * No atomics anywhere: two runs give the same bits.  Nothing allocates or synchronises.  1 <= H <= 256, N >= 1, B >= 1.
 * PHX_ERR_BAD_ARG before any device call for a null pointer (p, the parameter arrays a call reads, any array argument,
 * grads, grads->Ws / bs / Wp / bp, both of grads->Wa and grads->WaT, grads->g under overwrite) or a shape outside those
 * ranges.  PHX_ERR_WORKSPACE when workspace is null or workspace_bytes is below the call's *_workspace_bytes (0 for a shape
 * the call refuses). */
size_t phx_steady_adjoint_project_workspace_bytes(int N, int H, int B);
int phx_steady_adjoint_project(const phx_params *p, const float *m, const float *gy, int B, float *b, void *workspace,
                               size_t workspace_bytes, void *stream);
int phx_steady_adjoint_back(const phx_params *p, const float *y, const float *m, const float *gy, const float *q, const float *hid,
                            int B, float *lam, float *gy0, void *stream);
size_t phx_steady_param_grads_workspace_bytes(int N, int H, int B);
int phx_steady_param_grads(const phx_params *p, const float *y, const float *lam, const float *q, const float *hid, int B,
                           const phx_grads *grads, void *workspace, size_t workspace_bytes, void *stream);

/* The network of total effects at a fixed point (phoenix_amd.steady_state_response).  On the moving
 * genes r(y) + u = 0, so (I - M Wa C) dy = M du with M = diag(m), m = 1 on the genes that move in the row and 0 elsewhere,
 * and by the Woodbury identity of section 8o
 *     R = dy / du = M + M Wa Z C M,   Z = (I - S)^-1 (2H x 2H),   S = C M Wa   (phx_reduced_jacobian with this m).
 * Holding gene k and moving its level gives dy / d(level k) = R[:, k] / R[k, k].  phx_steady_resp.hip; all arrays on the
 * device, float unless said otherwise.
 * phx_steady_inverse: Z [B, 2H, 2H] float = (I - S_b)^-1, computed in double by LU with partial pivoting on [I - S | I],
 *   one workgroup per state, the pivot rule and the info codes of phx_steady_solve (0; k + 1: column k has no finite
 *   non-zero pivot; -1: the inverse is not finite as float; Z_b = 0 for both).  Workspace: phx_steady_inverse_workspace_bytes(H, B)
 *   = 2 B (2H)^2 doubles.
 * phx_steady_response_factors: for the K regulators genes[k] (int, 0 <= gene < N, device) and every state the column
 *   x_bk = Z_b C_b[:, gene] = a'(y) (Z_b[:, :H] Ws[:, gene]) + l'(y) ((Z_b[:, H:] diag hid_b[H:]) Wp[:, gene]), y = y[b, gene]:
 *   v_mfma_f32_16x16x4_f32 over the hidden index ascending, the two halves in accumulators of their own so that a' and l'
 *   are applied once per (b, k).  A second pass forms d_bk = 1 + m_bk sum_c WaT[c, gene] x_bk[c] (c ascending) and scales
 *   the column by m_bk (input 0, "production") or 1 / d_bk (input 1, "level").  X [B, 2H, K], use [B, K] (1.0: the row is
 *   used for this regulator; 0.0 where info[b] != 0 or d_bk is 0 or not finite: the column is then exactly 0).  A column
 *   of the weights that is exactly 0 gives an exactly-zero column.  K >= 1, B <= 65535.
 * phx_steady_response: out [K, N] (row stride ld >= N), out[k, j] = the mean over the used states of
 *   m_bj sum_c WaT[c, j] X_b[c, k] (absolute values where mean_abs != 0), plus m_bk on the diagonal j = genes[k] for input
 *   0; for input 1 the diagonal is exactly 1 (0 where no state is used).  The mean divides by sum_b use[b, k], read on the
 *   device (by 1 where that is 0).  One workgroup owns 64 regulators x 64 targets in accumulators over all the states and
 *   stores the tile once: no N x N temporary, no atomics; sums over c ascending, then b ascending; a regulator's row does
 *   not depend on the other regulators of the call.  X is walked 32 rows at a time through a double buffer in LDS, the
 *   chunk after the current one requested before the current one's products; the WaT panel stays in LDS where the whole
 *   workgroup stays within 64 KiB (H <= 64) and is streamed with the X chunks otherwise.  A target with m_bj = 0 gets an
 *   exact 0 from state b.
 * 1 <= H <= 256, N >= 1, B >= 1.  PHX_ERR_BAD_ARG before any device call for a null pointer, a shape outside the ranges, an
 * input outside {0, 1} or ld < N; PHX_ERR_WORKSPACE as above.  Nothing allocates or synchronises. */
size_t phx_steady_inverse_workspace_bytes(int H, int B);
int phx_steady_inverse(const float *S, int H, int B, float *Z, int *info, void *workspace, size_t workspace_bytes, void *stream);
int phx_steady_response_factors(const phx_params *p, const float *y, const float *m, const float *hid, const float *Z,
                                const int *info, int B, const int *genes, int K, int input, float *X, float *use, void *stream);
int phx_steady_response(const phx_params *p, const float *m, const float *X, const float *use, int B, const int *genes, int K,
                        int input, int mean_abs, float *out, long long ld, void *stream);

/* Diagnostic only (not part of the drop-in surface): with PHX_PROF=1 in the environment the v1 kernels
 * write 16 per-workgroup segment timers (100 MHz ticks) into the workspace; this returns where. */
/* Diagnostic only: the next phx_odeint / phx_odeint_adjoint_backward call on this thread records these two
 * hipEvent_t immediately before and after its solve kernel (not around its memset nodes / reduce kernel). */
void phx_debug_set_kernel_events(void *ev_start, void *ev_stop);
/* Diagnostic only: a process-wide FIFO of such pairs; every following phx_odeint / phx_odeint_adjoint_backward launch
 * (from any thread) takes the next pair.  (NULL, NULL) empties the queue.  Lets a bench time the solve kernels of
 * ordinary back-to-back training steps (forward on the caller's thread, backward on an autograd worker thread). */
void phx_debug_queue_kernel_events(void *ev_start, void *ev_stop);
int phx_debug_profile_region(int op, int N, int H, int B, int T, int control, size_t *offset,
                             int *n_workgroups, int *plan);
/* Diagnostic only: which backward-solve kernel phx_odeint_adjoint_backward launches for this shape:
 * 0 = k_solve_adj (VALU, grid barriers), 1 = k1_solve_adj (MFMA, one wave per trajectory tile),
 * 2 = k1_solve_adj2 (MFMA, wave pairs, fused sweeps), 3 = k1_solve_adj3 (MFMA, dopri5 with H <= 48: fused sweeps over
 * a 16-vector private state).  bench.py keys its profile lookups with it.  The first form assumes dopri5. */
int phx_debug_adjoint_kernel(int N, int H, int B, int T, int control);
int phx_debug_adjoint_kernel_m(int N, int H, int B, int T, int control, int method);
/* ... and which forward-solve kernel phx_odeint launches: 0 = k_solve_fwd (VALU), 1 = k1_solve_fwd (MFMA),
 * 3 = k1_solve_fwd3 (MFMA, dopri5 with H <= 48), 4 = k1_solve_fwd3c (its hidden-chunked form, 48 < H <= 256); the
 * adjoint query above likewise returns 4 for k1_solve_adj3c. */
int phx_debug_forward_kernel_m(int N, int H, int B, int T, int control, int method);
/* Both *_m queries: `method | 0x100` asks for the kernel of the stepped entry points (phx_odeint_stepped, ...); 0 then
 * means that no kernel with the sub-step loop plans the shape and the call returns PHX_ERR_BAD_ARG. */
/* Diagnostic only: how many launches of that solve kernel one call with this batch makes (a batch that does not fit one
 * residency is walked in chunks: e.g. 256 B-cell trajectories = two launches of k1_solve_adj3c).  op = PHX_OP_ODEINT or
 * PHX_OP_ADJOINT; 0 when no plan exists.  bench.py multiplies per-launch profile figures with it. */
int phx_debug_solve_launches(int op, int N, int H, int B, int T, int control, int method);
/* Diagnostic only, the calls-with-their-own-grids form of phx_odeint (B rows = `calls` calls of B / calls rows):
 * phx_debug_calls_grids_kernel_m: the kernel that serves it, numbered as by phx_debug_forward_kernel_m (1, 3 or 4; 0: none,
 *   the call returns PHX_ERR_BAD_ARG).
 * phx_debug_calls_grids_plan: returns the calls ONE launch takes (0: none) and, when `plan` is non-NULL, writes plan[0..5] =
 *   kernel, TG (batch groups = calls per launch), G (workgroups per group), NW (waves per workgroup), trajectory tiles per
 *   group, and the CU count the plan was sized for: TG * G <= plan[5] always.
 * phx_debug_calls_grids_launches: ceil(calls / calls per launch), the launches one phx_odeint call makes (0: none). */
int phx_debug_calls_grids_kernel_m(int N, int H, int B, int T, int calls, int method);
int phx_debug_calls_grids_plan(int N, int H, int B, int T, int calls, int method, int *plan);
int phx_debug_calls_grids_launches(int N, int H, int B, int T, int calls, int method);
/* Diagnostic only, needs no device: the plan of ONE launch of B rows by the solve kernel `kernel_id` of direction `op`
 * (PHX_OP_ODEINT: 1, 3, 4; PHX_OP_ADJOINT: 1 .. 4 and 5 = k1_solve_bp) on a device of `cus` compute units; calls > 1
 * (forward kernels): the rows are that many shared-control calls of B / calls rows.  Returns 0 where that kernel does
 * not plan the shape, else PHX_DEBUG_PLAN_FIELDS after writing out[0 .. PHX_DEBUG_PLAN_FIELDS - 1] =
 *   the launch geometry  N, H, B, T, HT, NB, NW, TPW, G, TG, nblk, ntg, Bt, nvec, BN, HC, Hc, Bcall, cntN, res, hb, split,
 *   the workspace layout (with gradients)  total, then the byte offsets cnt, part, zbuf, part1, zbuf1, scratch, dtheta,
 *     prof, wimg, hq, then xbytes (what a fill covers from `part` on), pp (floats per gradient partial), nparts,
 *   and the dynamic LDS bytes of the launch.
 * A planner change shows as the values it moves (tools/plan_table.py --cus, tests/golden/solve_plans.txt). */
#define PHX_DEBUG_PLAN_FIELDS 37
int phx_debug_plan(int op, int kernel_id, int cus, int N, int H, int B, int T, int control, int method, int calls,
                   long long *out);
/* Diagnostic only, needs no device: where a k1_solve_adj3 workspace says what became of the last step's quadrature.
 * *deferred = byte offset of one uint32 per batch group (1: the group left the visit of its last step to k3_tail_adj3 in
 * the workspace's latest launch, 0: it ran it itself), *served = byte offset of the uint32 in which the latest tail launch
 * left the number of deferred groups it worked on.  Returns 1 when the environment has the tail kernel on
 * (PHX_V3_TAIL=0 switches it off), else 0. */
int phx_debug_adj3_tail_words(size_t *deferred, size_t *served);

#ifdef __cplusplus
}
#endif
#endif
