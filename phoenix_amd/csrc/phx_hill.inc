// phx_hill.inc -- row f4 of SURVEY.md section 8: the ground-truth Hill-kinetics simulator the reference generates
// its in-silico data with (preprocessing_code/ground_truth_simulator/code: GraphGRN_core.R:425-486 builds one rate
// expression per gene -- shipped as ground_truth_simulator/clean_data/ode_system_functions_*.csv -- and
// SimulationGRN_core_init_var.R:218-247 integrates them per sample with deSolve::ode).
//
// The host (phoenix_amd/simulator.py) compiles every gene's expression into a postfix program over
//   PUSHC c | PUSHX gene | ADD | SUB | MUL | DIV | NEG | FACT(B, K_n, n)
// with fAct(TF, EC50, n) = B TF^n / (K_n + TF^n), B = (EC50^n - 1) / (2 EC50^n - 1), K_n = B - 1
// (GraphGRN_core.R:431-436); "input gene" rows have rate 0.  One thread interprets one gene's program.
namespace {

enum { HOP_PUSHC = 0, HOP_PUSHX = 1, HOP_ADD = 2, HOP_SUB = 3, HOP_MUL = 4, HOP_DIV = 5, HOP_NEG = 6, HOP_FACT = 7 };
constexpr int HILL_STACK = 24;

struct HillProg {
    const int2 *code;      // (op, arg)
    const int *off, *len;  // per gene
    const float *consts;   // PUSHC: consts[arg]; FACT: consts[arg .. arg+2] = B, K_n, n
};

__device__ __forceinline__ float hill_eval(const HillProg &p, int gene, const float *x)
{
    float st[HILL_STACK];
    int sp = 0;
    const int2 *c = p.code + p.off[gene];
    const int n = p.len[gene];
    for (int i = 0; i < n; ++i) {
        const int2 ins = c[i];
        switch (ins.x) {
            case HOP_PUSHC: st[sp++] = p.consts[ins.y]; break;
            case HOP_PUSHX: st[sp++] = x[ins.y]; break;
            case HOP_ADD: sp--; st[sp - 1] = st[sp - 1] + st[sp]; break;
            case HOP_SUB: sp--; st[sp - 1] = st[sp - 1] - st[sp]; break;
            case HOP_MUL: sp--; st[sp - 1] = st[sp - 1] * st[sp]; break;
            case HOP_DIV: sp--; st[sp - 1] = st[sp - 1] / st[sp]; break;
            case HOP_NEG: st[sp - 1] = -st[sp - 1]; break;
            default: {   // HOP_FACT
                const float B = p.consts[ins.y], K = p.consts[ins.y + 1], nn = p.consts[ins.y + 2];
                const float tf = st[sp - 1];
                const float tn = tf > 0.f ? powf(tf, nn) : 0.f;
                st[sp - 1] = B * tn / (K + tn);
            }
        }
    }
    return n > 0 ? st[0] : 0.f;
}

__global__ void k_hill_rhs(HillProg p, const float *__restrict__ x, float *__restrict__ out, int B, int N)
{
    const int gene = blockIdx.x * blockDim.x + threadIdx.x;
    if (gene >= N) return;
    // rows are strided over gridDim.y (capped by the host), so B is not bounded by the 65 535 limit of a grid's y dimension
    for (int b = blockIdx.y; b < B; b += gridDim.y) out[(long long)b * N + gene] = hill_eval(p, gene, x + (long long)b * N);
}

// One workgroup per sample, the sample's state in LDS, classical RK4 with equal sub-steps <= dt_max between the
// requested output times (the reference calls lsoda; the tests compare against a tight-tolerance CPU solve).
constexpr int HILL_GPT = 8;   // genes per thread (N <= 8 * 1024)
__global__ __launch_bounds__(1024) void k_hill_simulate(HillProg p, const float *__restrict__ x0,
                                                        const double *__restrict__ times, int T, double dt_max,
                                                        float *__restrict__ out, int B, int N)
{
    extern __shared__ float xs[];
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    float y[HILL_GPT], acc[HILL_GPT], k[HILL_GPT];
#pragma unroll
    for (int g = 0; g < HILL_GPT; ++g) {
        const int gene = tid + g * nt;
        y[g] = gene < N ? x0[(long long)b * N + gene] : 0.f;
        if (gene < N) { xs[gene] = y[g]; out[(long long)b * N + gene] = y[g]; }
    }
    __syncthreads();
    auto stage = [&](float wk, float hnext, bool last) {   // k = f(xs); acc += wk k; xs = y + hnext k (or new y)
#pragma unroll
        for (int g = 0; g < HILL_GPT; ++g) {
            const int gene = tid + g * nt;
            k[g] = gene < N ? hill_eval(p, gene, xs) : 0.f;
            acc[g] += wk * k[g];
        }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < HILL_GPT; ++g) {
            const int gene = tid + g * nt;
            if (last) y[g] = y[g] + hnext * acc[g];
            if (gene < N) xs[gene] = last ? y[g] : y[g] + hnext * k[g];
        }
        __syncthreads();
    };
    for (int i = 0; i + 1 < T; ++i) {
        const double span = times[i + 1] - times[i];
        const int nsub = max(1, (int)ceil(fabs(span) / dt_max));
        const float h = (float)(span / nsub);
        for (int s = 0; s < nsub; ++s) {
#pragma unroll
            for (int g = 0; g < HILL_GPT; ++g) acc[g] = 0.f;
            stage(1.f, 0.5f * h, false);
            stage(2.f, 0.5f * h, false);
            stage(2.f, h, false);
            stage(1.f, h / 6.f, true);
        }
#pragma unroll
        for (int g = 0; g < HILL_GPT; ++g) {
            const int gene = tid + g * nt;
            if (gene < N) out[((long long)(i + 1) * B + b) * N + gene] = y[g];
        }
    }
}

}  // namespace
