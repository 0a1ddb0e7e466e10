// The optimiser: fused multi-tensor AdamW with its C entries, the host scalars every AdamW kernel of the library is fed
// (gd_adam_hyper), and the graph step state -- the device block that carries those scalars and the Philox offsets when a training
// step is replayed from a hipGraph.
#include <math.h>
#include <stdlib.h>

#include "common.h"

namespace {

// fused multi-tensor AdamW (torch.optim.AdamW single-tensor math, reference main.py:258,351)
constexpr int ADAM_BLOCK_ELEMS = 4096;

// stab (optional): [n][3] = (bf16 shadow pointer or 0, columns, shadow row stride) -- the updated parameter is also
// stored, rounded to bfloat16, into its zero-padded 2-D shadow (gdmcf_bf16_shadow_set)
template <bool NT_>
__global__ __launch_bounds__(256) void adamw_kernel(const int64_t* __restrict__ table, int n_tensors,
                                                    GdAdamHyper h, const int64_t* __restrict__ stab, const GdStepState* step_state) {
    if (step_state) h = step_state->hyper;  // graph mode: this step's scalars from the device
    int t = 0;
    for (int i = 1; i < n_tensors; ++i)
        if ((int64_t)blockIdx.x >= table[i * 6 + 5]) t = i;
    float* p = reinterpret_cast<float*>(table[t * 6 + 0]);
    const float* g = reinterpret_cast<const float*>(table[t * 6 + 1]);
    float* m = reinterpret_cast<float*>(table[t * 6 + 2]);
    float* v = reinterpret_cast<float*>(table[t * 6 + 3]);
    const int64_t n = table[t * 6 + 4];
    const int64_t base = ((int64_t)blockIdx.x - table[t * 6 + 5]) * ADAM_BLOCK_ELEMS;
    const bool al = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                      reinterpret_cast<uintptr_t>(v)) & 15u) == 0;
    unsigned short* p16 = stab ? reinterpret_cast<unsigned short*>(stab[t * 3 + 0]) : nullptr;
    const unsigned cols16 = p16 ? (unsigned)stab[t * 3 + 1] : 1u;
    const int64_t ld16 = p16 ? stab[t * 3 + 2] : 0;
#pragma unroll
    for (int it = 0; it < ADAM_BLOCK_ELEMS / (256 * 4); ++it) {
        const int64_t i = base + (int64_t)(it * 256 + threadIdx.x) * 4;
        if (al && i + 3 < n) {
            f32x4 pp, gg, mm, vv;
            if (NT_) {
                pp = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(p + i));
                gg = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + i));
                mm = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(m + i));
                vv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(v + i));
            } else {
                pp = *reinterpret_cast<f32x4*>(p + i);
                gg = *reinterpret_cast<const f32x4*>(g + i);
                mm = *reinterpret_cast<f32x4*>(m + i);
                vv = *reinterpret_cast<f32x4*>(v + i);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float pj = pp[j], mj = mm[j], vj = vv[j];
                gd_adam_elem(pj, gg[j], mj, vj, h);
                pp[j] = pj;
                mm[j] = mj;
                vv[j] = vj;
            }
            if (NT_) {
                __builtin_nontemporal_store(pp, reinterpret_cast<f32x4*>(p + i));
                __builtin_nontemporal_store(mm, reinterpret_cast<f32x4*>(m + i));
                __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(v + i));
            } else {
                *reinterpret_cast<f32x4*>(p + i) = pp;
                *reinterpret_cast<f32x4*>(m + i) = mm;
                *reinterpret_cast<f32x4*>(v + i) = vv;
            }
            if (p16) {
                unsigned r = (unsigned)i / cols16, c = (unsigned)i - r * cols16;  // numel < 2^32 (checked on the host)
                if (c + 3 < cols16) {
                    // one 8-byte store; only 2-byte aligned when the row length is odd (gfx950 runs with unaligned
                    // global access enabled, hipcc emits global_store_dwordx2 for it)
                    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
                    typedef u32x2 u32x2_u __attribute__((aligned(2)));
                    const u32x2 w = {gd_bf16_bits(pp[0]) | ((unsigned)gd_bf16_bits(pp[1]) << 16),
                                     gd_bf16_bits(pp[2]) | ((unsigned)gd_bf16_bits(pp[3]) << 16)};
                    *reinterpret_cast<u32x2_u*>(p16 + (int64_t)r * ld16 + c) = w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        p16[(int64_t)r * ld16 + c] = gd_bf16_bits(pp[j]);
                        if (++c == cols16) {
                            c = 0;
                            ++r;
                        }
                    }
                }
            }
        } else {
            for (int j = 0; j < 4; ++j)
                if (i + j < n) {
                    gd_adam_elem(p[i + j], g[i + j], m[i + j], v[i + j], h);
                    if (p16) {
                        const unsigned r = (unsigned)(i + j) / cols16, c = (unsigned)(i + j) - r * cols16;
                        p16[(int64_t)r * ld16 + c] = gd_bf16_bits(p[i + j]);
                    }
                }
        }
    }
}

}  // namespace

// The C ABI carries the hyper-parameters as float; torch.optim.AdamW forms its scalars from the Python doubles the user wrote
// (1 - 0.999 = 0.001, whereas 1 - (double)0.999f = 0.00099998713: 1.3e-5 off in every exp_avg_sq increment).  The double the
// user meant is the shortest decimal that rounds to the float we were given (7 significant digits identify a float).
static double gd_decimal(float x) {
    char buf[32];
    snprintf(buf, sizeof buf, "%.7g", (double)x);
    const double d = strtod(buf, nullptr);
    return (float)d == x ? d : (double)x;
}

GdAdamHyper gd_adam_hyper(float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale) {
    // scalars formed in double exactly as torch/optim/adamw.py does, then narrowed to f32
    GdAdamHyper h;
    const double lr_d = gd_decimal(lr), b1 = gd_decimal(beta1), b2 = gd_decimal(beta2), wd = gd_decimal(weight_decay);
    const double bc1 = 1.0 - pow(b1, (double)step);
    const double bc2 = 1.0 - pow(b2, (double)step);
    h.decay = (float)(1.0 - lr_d * wd);
    h.one_m_b1 = (float)(1.0 - b1);
    h.beta2 = beta2;
    h.one_m_b2 = (float)(1.0 - b2);
    h.bc2_sqrt = (float)sqrt(bc2);
    h.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    h.eps = eps;
    h.neg_step = (float)(-(lr_d / bc1));
    h.grad_scale = grad_scale;
    return h;
}

extern "C" {

static int adamw_launch(const int64_t* table, const int64_t* shadow_table, int n_tensors, int total_blocks, float lr,
                        float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                        void* stream) {
    GD_CHECK_ARG(n_tensors > 0 && total_blocks > 0 && step >= 1, "adamw: bad arguments");
    const GdAdamHyper h = gd_adam_hyper(lr, beta1, beta2, eps, weight_decay, step, grad_scale);
    {
        // algorithmic bytes: read p, g, m, v; write p, m, v (+ the 2-byte shadow of p in bf16 mode)
        GdProfScope prof(6, (shadow_table ? 30.0 : 28.0) * ADAM_BLOCK_ELEMS * (double)total_blocks, (hipStream_t)stream);
        // nontemporal accesses for the streamed optimiser state: A/B on one box 0.344 -> 0.318 ms at the Yelp shape,
        // 1.032 -> 0.911 ms at the Amazon-Book shape (GDMCF_ADAMW_NT=0 switches back for comparison runs)
        static const bool nt = gd_env_int("GDMCF_ADAMW_NT", 1) != 0;
        if (nt)
            hipLaunchKernelGGL(adamw_kernel<true>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, table, n_tensors, h,
                               shadow_table, t_gd_step_state);
        else
            hipLaunchKernelGGL(adamw_kernel<false>, dim3(total_blocks), dim3(256), 0, (hipStream_t)stream, table, n_tensors,
                               h, shadow_table, t_gd_step_state);
    }
    return gd_launch_status("adamw");
}

int gdmcf_adamw_f32(const int64_t* table, int n_tensors, int total_blocks, float lr, float beta1, float beta2,
                    float eps, float weight_decay, int step, float grad_scale, void* stream) {
    return adamw_launch(table, nullptr, n_tensors, total_blocks, lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                        stream);
}

int gdmcf_adamw_bf16s_f32(const int64_t* table, const int64_t* shadow_table, int n_tensors, int total_blocks, float lr,
                          float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                          void* stream) {
    GD_CHECK_ARG(shadow_table != nullptr, "adamw_bf16s: shadow table missing");
    return adamw_launch(table, shadow_table, n_tensors, total_blocks, lr, beta1, beta2, eps, weight_decay, step,
                        grad_scale, stream);
}

}  // extern "C"

// ---- graph step state ---------------------------------------------------------------------------------------------------
thread_local const GdStepState* t_gd_step_state = nullptr;

__global__ void graph_state_tick_kernel(GdStepState* st) {
    st->prep_offset += 1;
    st->ts_offset += 1;
    st->adam_step += 1;
    int64_t k = st->adam_step - st->table_first;
    k = k < 0 ? 0 : (k >= st->table_len ? st->table_len - 1 : k);  // the host refills the table before it runs out
    st->hyper = st->hyper_table[k];
}

extern "C" {

int gdmcf_graph_state_bytes(void) { return (int)sizeof(GdStepState); }
int gdmcf_adam_hyper_bytes(void) { return (int)sizeof(GdAdamHyper); }

int gdmcf_graph_state_bind(const void* state_dev) {
    t_gd_step_state = static_cast<const GdStepState*>(state_dev);
    return GDMCF_OK;
}

int gdmcf_graph_state_init(void* state_host, uint64_t prep_offset, uint64_t ts_offset, int64_t adam_step, int64_t table_first,
                           int64_t table_len, const void* hyper_table_dev) {
    GD_CHECK_OFFSET(prep_offset | ts_offset, "graph_state_init");
    GD_CHECK_ARG(state_host && hyper_table_dev && table_len > 0, "graph_state_init: null pointer / empty table");
    GdStepState* st = static_cast<GdStepState*>(state_host);
    st->prep_offset = prep_offset; st->ts_offset = ts_offset; st->adam_step = adam_step; st->table_first = table_first;
    st->table_len = table_len; st->hyper_table = static_cast<const GdAdamHyper*>(hyper_table_dev);
    st->hyper = GdAdamHyper{};
    return GDMCF_OK;
}

int gdmcf_adam_hyper_fill(void* out_host, int n, float lr, float beta1, float beta2, float eps, float weight_decay,
                          int64_t first_step, float grad_scale) {
    GD_CHECK_ARG(out_host && n > 0 && first_step >= 1, "adam_hyper_fill: bad arguments");
    GdAdamHyper* o = static_cast<GdAdamHyper*>(out_host);
    for (int k = 0; k < n; ++k) o[k] = gd_adam_hyper(lr, beta1, beta2, eps, weight_decay, (int)(first_step + k), grad_scale);
    return GDMCF_OK;
}

int gdmcf_graph_state_tick(void* state_dev, void* stream) {
    GD_CHECK_ARG(state_dev, "graph_state_tick: null state");
    hipLaunchKernelGGL(graph_state_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, static_cast<GdStepState*>(state_dev));
    return gd_launch_status("graph_state_tick");
}

}  // extern "C"
