// phx_host.hpp -- host-side helpers shared by the translation units of libphoenix_hip.so.
// Inline variables (C++17): one instance per shared library, whichever TU references them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <utility>
#include <vector>

#include "phx_solver.hpp"

namespace phxh {

// CU count of the CURRENT device (cached per device ordinal)
inline std::mutex g_mu;
inline std::map<int, int> g_cus;
inline int num_cus()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_cus.find(dev);
    if (it != g_cus.end()) return it->second;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    g_cus[dev] = n;
    return n;
}

// Raises the dynamic-LDS limit of a kernel.  hipFuncAttributeMaxDynamicSharedMemorySize is a per-device, per-function
// attribute: the cache is keyed by (device, function pointer) and guarded by a mutex; the driver call is made only
// when a launch needs more than was granted before.
inline std::map<std::pair<int, const void *>, size_t> g_lds_granted;
inline bool set_lds_fn(const void *fn, size_t bytes)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    std::lock_guard<std::mutex> lk(g_mu);
    auto key = std::make_pair(dev, fn);
    auto it = g_lds_granted.find(key);
    if (it != g_lds_granted.end() && it->second >= bytes) return true;
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    g_lds_granted[key] = bytes;
    return true;
}
template <typename K>
inline bool set_lds(K kernel, size_t bytes) { return set_lds_fn(reinterpret_cast<const void *>(kernel), bytes); }

// Co-residency guard of the persistent kernels (they spin on each other's rows): the launch is refused unless the
// occupancy query says that `grid` workgroups of this shape fit the device at once.  Cached per (device, fn, threads, lds).
inline std::map<std::tuple<int, const void *, int, size_t>, int> g_occ;
inline bool fits_resident(const void *fn, int threads, size_t lds, int grid)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    int per_cu = -1;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_occ.find(std::make_tuple(dev, fn, threads, lds));
        if (it != g_occ.end()) per_cu = it->second;
    }
    if (per_cu < 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, lds) != hipSuccess) return false;
        per_cu = n;
        std::lock_guard<std::mutex> lk(g_mu);
        g_occ[std::make_tuple(dev, fn, threads, lds)] = per_cu;
    }
    return (long long)per_cu * num_cus() >= grid;
}

// persistent kernels: LDS limit + co-residency check in one call (PHX_ERR_LAUNCH instead of a grid that would spin)
template <typename K>
inline bool set_lds_resident(K kernel, size_t bytes, int threads, int grid)
{
    const void *fn = reinterpret_cast<const void *>(kernel);
    return set_lds_fn(fn, bytes) && fits_resident(fn, threads, bytes, grid);
}

// Persistent kernels whose workgroups wait for each other's rows need the whole grid resident at once.  Two ways to get
// that: (default) a plain launch behind the occupancy check of fits_resident -- the library refuses a grid the device
// cannot hold, and the engine's stream must not share the device with another long-running kernel (launch
// planning); or PHX_COOP=1: hipLaunchCooperativeKernel, where the runtime itself guarantees co-residency.  The
// cooperative path is NOT the default because it costs 18-19 us per launch on this stack (C4, same box, round 4:
// forward 0.286 vs 0.268 ms, backward 0.616 vs 0.598 ms, step 0.939 vs 0.892 ms); it is there for deployments that
// cannot keep other long kernels off the device.
inline bool use_coop()
{
    const char *e = getenv("PHX_COOP");
    return e && e[0] == '1';
}
template <typename... Args>
inline hipError_t launch_persistent(const void *fn, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args)
{
    void *argv[] = {(void *)&args...};
    if (use_coop()) return hipLaunchCooperativeKernel(fn, grid, block, argv, (unsigned int)lds, st);
    return hipLaunchKernel(fn, grid, block, argv, lds, st);
}
// the plain launch of the older persistent kernels (k1_solve_fwd / adj / adj2: never cooperative); `args` must carry the
// kernel's parameter types exactly
template <typename... Args>
inline hipError_t launch_plain(const void *fn, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args)
{
    void *argv[] = {(void *)&args...};
    return hipLaunchKernel(fn, grid, block, argv, lds, st);
}

// diagnostic: optional HIP events recorded immediately around the next solve kernel (bench.py roofline timing)
inline thread_local hipEvent_t g_ev_start = nullptr, g_ev_stop = nullptr;
// ... and a process-wide FIFO of such pairs (phx_debug_queue_kernel_events): successive solve launches take one pair each,
// whichever thread issues them (the backward solve of a training step runs on an autograd worker thread), so a bench can
// time the kernels of ordinary back-to-back steps instead of isolated launches
inline std::mutex g_evq_mu;
inline std::vector<std::pair<hipEvent_t, hipEvent_t>> g_evq;
inline void ev_begin(hipStream_t st)
{
    if (!g_ev_start) {
        std::lock_guard<std::mutex> lk(g_evq_mu);
        if (!g_evq.empty()) {
            g_ev_start = g_evq.front().first;
            g_ev_stop = g_evq.front().second;
            g_evq.erase(g_evq.begin());
        }
    }
    if (g_ev_start) (void)hipEventRecord(g_ev_start, st);
}
inline void ev_end(hipStream_t st)
{
    if (g_ev_stop) (void)hipEventRecord(g_ev_stop, st);
    g_ev_start = nullptr;
    g_ev_stop = nullptr;
}

inline Net to_net(const phx_params *p) { return Net{p->Ws, p->bs, p->Wp, p->bp, p->WaT, p->g, p->N, p->H}; }

constexpr size_t LDS_BUDGET = 163840 - 1024;

inline bool force_v0()
{
    const char *e = getenv("PHX_ENGINE");
    return e && strcmp(e, "v0") == 0;
}

}  // namespace phxh

// ---- persistent solve kernels (k1_solve_fwd / fwd3 / fwd3c, k1_solve_adj / adj2 / adj3 / adj3c): one description per
// kernel family, defined by the family's translation unit; phx_engine.hip picks the family and drives its launches
namespace phxh {

// workspace layout of one plan: byte offsets of the regions every family draws from (a region a family does not use has
// zero bytes), in the one order of make_regions (phx_plan.hpp)
struct Regions {
    size_t total, cnt, part, zbuf, part1, zbuf1, scratch, dtheta, prof, wimg, hq;
    size_t xbytes;      // bytes from `part` on that a fill zeroes together with the header [cnt, part)
    long long pp;       // backward: floats per gradient partial
    int nparts;         // backward: partials the gradient reduce sums
};

// one launch: the arguments the solve kernels take, pointers already offset to the launch's rows
struct SolveArgs {
    Net net;
    D1 d;
    W1 w;
    SolveCfg cfg;
    size_t lds;
    const double *t;
    const float *y0, *y_saved, *grad_y;   // forward: y0; backward: y_saved, grad_y
    float *sol, *adj_y0;
    int *status, *nfe, *nsteps;
    int grads;            // backward: 1 = parameter gradients wanted
    long long PP;         // backward: Regions::pp
    float *ckpt;          // k1_solve_bp: checkpoint region [D1::K][rows of the launch][N] (null: none)
    const int *clamp;     // phx_odeint_clamped_sets: the held genes of each call of the launch (device, [D1::TG, clamp_width]);
                          // null: none
    int clamp_width;      // ... and the entries per call (1 .. PHX_CLAMP_MAX)
};

// what a launch is planned for: the CUs that must hold its workgroups at once, the batch of B rows with T time points,
// step control and method, and calls > 1: B = calls x (B / calls) rows of independent shared-control dopri5 calls that
// share the launch (forward kernels only, D1::Bcall); calls == 1: the ordinary plan
struct Shape {
    int cus, N, H, B, T, control, method, calls;
};

struct Backend {
    int id;                    // kernel generation phx_debug_{forward,adjoint}_kernel_m report (1 .. 4; k1_solve_bp: 5)
    bool cleans_idle_set;      // the kernel cleans its idle exchange set: ws_keep may skip the fill of a one-launch batch
    bool zero_dtheta_always;   // gradient partials are zeroed before every launch, else only when T < 2 (nobody steps)
    bool prof_levels;          // PHX_PROF=<level >= 1> turns the timers on; else only a value that starts with '1'
    bool (*plan)(const Shape &s, D1 *out);   // a pure function of the shape and the switches (phx_plan.hpp)
    Regions (*layout)(const D1 &d, bool grads);
    size_t (*lds)(const D1 &d);   // dynamic LDS bytes of the launch
    int (*plan6)(const D1 &d);   // last entry of phx_debug_profile_region's plan
    // the images (packed into a.w.wimg unless the caller's serve) and the kernel; null: no kernel for this plan
    const void *(*prepare)(SolveArgs &a, const phx_params *p, hipStream_t st);
    hipError_t (*launch)(const void *fn, const SolveArgs &a, hipStream_t st);
    // backward: sums `npart` partials into the caller's gradients; false on a launch error
    bool (*reduce)(const SolveArgs &a, int npart, const phx_grads *g, int overwrite, hipStream_t st);
    bool substeps = false;     // the fixed-grid arm takes the sub-steps of options["step_size"] (SolveCfg::step)
};

// the layouts' allocator: regions 256-byte aligned, in the order they are taken
struct Take {
    size_t off = 0;
    size_t operator()(size_t bytes)
    {
        const size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    }
};

// plan[5] of phx_debug_profile_region: the hidden tiles, or for the hidden-chunked kernels HC*10 + res + 2 hb + 4 split
inline int plan6_ht(const D1 &d) { return d.HT; }
inline int plan6_chunked(const D1 &d) { return d.HC * 10 + d.res + 2 * d.hb + (d.split > 1 ? 4 : 0); }

// (functions: a host object at namespace scope that holds host function pointers breaks the device link)
const Backend &fwd3_backend();
const Backend &fwd3c_backend();
const Backend &adj2_backend();
const Backend &adj3_backend();
const Backend &adj3c_backend();
// k1_solve_bp (backpropagation through the fixed-grid steps): not in the lists of the adjoint direction, it has entry
// points of its own
const Backend &bp_backend();

// k3_tail_adj3 (phx_adj3t.hip), launched behind k1_solve_adj3 in place of its gradient reduce: adj3_tail_on says whether
// this launch runs with it (the solve kernel then may defer its last visit, and the reduce step launches the tail)
bool adj3_tail_on(const SolveArgs &a);
bool launch_adj3_tail(const SolveArgs &a, const phx_grads *g, int overwrite, hipStream_t st);

// the CALLS + CLAMP forms of k1_solve_fwd3 / k1_solve_fwd3c (phx_odeint_clamped), compiled in units of their own
// (phx_fwd3k.hip, phx_fwd3ck.hip) so that the parallel build is no longer than before
const void *fwd3_clamp_kernel(bool half);
const void *fwd3c_clamp_kernel(int nbt, bool half, bool hb);

// the CLAMP forms with a held set per trajectory ROW (phx_odeint_clamped_rows, phx_odeint_adjoint_backward_clamped_rows),
// in units of their own too: k1_solve_fwd3's (phx_fwd3r.hip; phx_fwd3.hip's backend launches them) and k1_solve_adj3's
// (phx_adj3r.hip), which come with a backend of their own -- k1_solve_adj3 at EVERY shape its planner lays out, also the
// small gene-tile groups that an unclamped solve leaves to k1_solve_adj2, and always without the tail kernel
const void *fwd3_rows_kernel(bool half, bool split);
const Backend &adj3_rows_backend();
// phx_adj3.hip's planner without its choice between k1_solve_adj3 and k1_solve_adj2
bool plan_adj3_any(const Shape &s, D1 *out);

}  // namespace phxh
