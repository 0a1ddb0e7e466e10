// Noise written to memory: the one-hot image under the discrete transition noise, the N(0,1) fill, the eps loss target and the
// degree-guided graph step of the reverse loop -- each kernel with its C entry.  The draws themselves are draws.h's, shared bit
// for bit with the input builders (prep_input.hip, cat.hip) that form the same values in place.
#include "draws.h"

namespace {

// One-hot rows with discrete transition noise (reference gaussian_diffusion.py:770-831 with :597-614, :999-1038, and the
// `x_tU & one_hot(x_start)` of :849 / :686): item i of row b has class c0 = x0[b,i]; a class s is drawn from row c0 of
// Q = a*I + (1-a)*[[e,1-e],[e,1-e]], a = (float)ts[b] / B (the reference's own scaling, :775); the pair written is
// (c0==0 && s==0, c0==1 && s==1), i.e. the true class's bit survives only where the draw reproduces it.
// Four items per thread: one Philox block (stream 3) gives their four uniforms.
__global__ __launch_bounds__(256) void onehot_noise_kernel(const float* __restrict__ x0, int64_t ldx,
                                                          const int64_t* __restrict__ ts, int B, int I, float p1_off,
                                                          const uint8_t* __restrict__ sampled, int64_t lds, uint64_t seed,
                                                          uint64_t offset, float* __restrict__ xU, int64_t ldu,
                                                          uint8_t* __restrict__ sampled_out, int64_t ldso) {
    const int b = blockIdx.y;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= I) return;
    uint32_t u[4] = {0u, 0u, 0u, 0u};
    float a = 1.f;
    if (!sampled) {
        const uint4 r = gd_philox_block((uint32_t)(i0 >> 2), b, GD_STREAM_ONEHOT_CLASS, offset, gd_philox_key(seed));
        u[0] = r.x; u[1] = r.y; u[2] = r.z; u[3] = r.w;
        a = gd_class_scale(ts[b], B);
    }
    const bool full = i0 + 3 < I;
    float xv[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t sv = 0;  // given classes of the four items, one per byte
    if (full) {  // (the rolled ragged loop below is this kernel's own form: gd_load4's unrolled tail costs it a different schedule)
        const f32x4 t4 = *reinterpret_cast<const f32x4_u4*>(x0 + (int64_t)b * ldx + i0);
        xv[0] = t4.x; xv[1] = t4.y; xv[2] = t4.z; xv[3] = t4.w;
    } else {
        for (int j = 0; j < 4; ++j)
            if (i0 + j < I) xv[j] = x0[(int64_t)b * ldx + i0 + j];
    }
    if (sampled)
        for (int j = 0; j < 4; ++j)
            if (i0 + j < I) sv |= (uint32_t)(sampled[(int64_t)b * lds + i0 + j] != 0) << (8 * j);
    float o[8];
    uint32_t so = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c0 = xv[j] != 0.f;
        int s;
        if (sampled) {
            s = (sv >> (8 * j)) & 1;
        } else {
            s = gd_class_draw(c0, a, p1_off, u[j]);
        }
        so |= (uint32_t)s << (8 * j);
        const float keep = (s == c0) ? 1.f : 0.f;
        o[2 * j] = c0 ? 0.f : keep;
        o[2 * j + 1] = c0 ? keep : 0.f;
    }
    float* op = xU + (int64_t)b * ldu + 2 * (int64_t)i0;
    if (full) {
        *reinterpret_cast<f32x4_u4*>(op) = f32x4{o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4_u4*>(op + 4) = f32x4{o[4], o[5], o[6], o[7]};
    } else {
        for (int j = 0; j < 4; ++j)
            if (i0 + j < I) {
                op[2 * j] = o[2 * j];
                op[2 * j + 1] = o[2 * j + 1];
            }
    }
    if (sampled_out)
        for (int j = 0; j < 4; ++j)
            if (i0 + j < I) sampled_out[(int64_t)b * ldso + i0 + j] = (uint8_t)((so >> (8 * j)) & 1);
}

// N(0,1) fill (reference gaussian_diffusion.py:328-331 `noise = th.randn_like(x_start)` when eps is the TARGET and so has to
// exist in memory, :210-217 the reverse loop's `noise = th.randn_like(x_t)`): the SAME normals the input builder draws in
// place (noise_mode 2) for the same (seed, offset) when stream == 0 -- element (b, i) is normal i & 3 of the block with
// counter (i >> 2, b, stream, offset), gd_normal4 -- so a row written here and handed to the builder
// as given noise reproduces the in-kernel stream bit for bit.  Four elements per thread, 16-byte stores where the row allows.
__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, int64_t ld, int rows, int cols, uint32_t stream,
                                                   uint64_t seed, uint64_t offset) {
    const int b = blockIdx.y;
    const uint2 key = gd_philox_key(seed);
    float* __restrict__ orow = out + (int64_t)b * ld;
#pragma unroll
    for (int u = 0; u < PREP_G; ++u) {
        const int col = (blockIdx.x * (256 * PREP_G) + u * 256 + threadIdx.x) * 4;
        if (col >= cols) return;
        float z[4];
        // gd_normal4, its two halves written out: behind one more call level hipcc orders four xor operands of the last Philox
        // round differently, and this kernel's instructions are to stay what they were
        gd_block_normals(philox4x32_10(gd_normal_counter(col, b, stream, offset), key), z);
        if (col + 3 < cols) {
            *reinterpret_cast<f32x4_u4*>(orow + col) = f32x4{z[0], z[1], z[2], z[3]};
        } else {
            for (int j = 0; j < 4; ++j)
                if (col + j < cols) orow[col + j] = z[j];
        }
    }
}

// Loss target of the eps parameterisation (reference gaussian_diffusion.py:344-348): target = eps, except rows with t == 0
// (when the x0-likelihood term is on) whose target is r1[0]*x_t - x0 with weight r2[0] on the model output and twice the
// divisor.  target may BE the noise buffer: then only the t == 0 rows are touched (a few KB instead of three [B, I] passes).
// The product and the difference are rounded separately, as torch's mul and sub are.
__global__ __launch_bounds__(256) void eps_target_kernel(const float* __restrict__ noise, int64_t ldn, const float* __restrict__ xt,
                                                        int64_t ldxt, const float* __restrict__ x0, int64_t ldx0,
                                                        const int64_t* __restrict__ ts, const float* __restrict__ r1,
                                                        const float* __restrict__ r2, int t0_likelihood, int I,
                                                        float* target, int64_t ldt, float* __restrict__ alpha,
                                                        float* __restrict__ rowdiv) {
    const int b = blockIdx.y;
    const bool is0 = t0_likelihood && ts[b] == 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        alpha[b] = is0 ? r2[0] : 1.f;
        rowdiv[b] = is0 ? 2.f * (float)I : (float)I;
    }
    if (!is0 && target == noise) return;
    const float c = r1[0];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < I; i += gridDim.x * 256) {
        float v;
        if (is0) {
#pragma clang fp contract(off)
            const float p = c * xt[(int64_t)b * ldxt + i];
            v = p - x0[(int64_t)b * ldx0 + i];
        } else {
            v = noise[(int64_t)b * ldn + i];
        }
        target[(int64_t)b * ldt + i] = v;
    }
}

// degree-guided graph of the reverse loop (reference gaussian_diffusion.py:706-729): per reverse step the reference
// draws a class for every (user, item) from row c of Q_bar(t / batch) where c is the edge's state so far
// (apply_noise on the accumulated one-hot graph), draws ONE bit per user from [1 - deg/maxdeg, deg/maxdeg]
// (multinomial(1)), ANDs the two when args.user_guided and ORs the result into the graph.  As bits:
//   graph[b,i] |= s[b,i] & (user_guided ? pick[b] : 1),   s ~ (u < a*[c == 1] + (1 - a)*(1 - e)),  a = (float)ts[b]/B.
// One byte per edge state, four items per thread; Philox4x32-10 streams 5 (classes) and 6 (user bits).
__global__ __launch_bounds__(256) void graph_step_kernel(uint8_t* __restrict__ graph, int64_t ldg, const int64_t* __restrict__ ts,
                                                        int B, int I, float p1_off, const uint8_t* __restrict__ sampled,
                                                        int64_t lds, const uint8_t* __restrict__ pick_in,
                                                        const float* __restrict__ degp, int user_guided, uint64_t seed,
                                                        uint64_t offset, uint8_t* __restrict__ sampled_out, int64_t ldso,
                                                        uint8_t* __restrict__ pick_out) {
    const int b = blockIdx.y;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    const uint2 key = gd_philox_key(seed);
    int pick = 1;
    if (pick_in) {
        pick = pick_in[b] != 0;
    } else if (degp) {  // one draw per user, the same in every thread of the row
        const uint4 r = gd_philox_block(0xFFFFFFFFu, b, GD_STREAM_GRAPH_PICK, offset, key);
        pick = gd_uniform24(r.x) < degp[b];
    }
    if (pick_out && blockIdx.x == 0 && threadIdx.x == 0) pick_out[b] = (uint8_t)pick;
    if (i0 >= I) return;
    uint32_t u[4] = {0u, 0u, 0u, 0u};
    float a = 1.f;
    if (!sampled) {
        const uint4 r = gd_philox_block((uint32_t)(i0 >> 2), b, GD_STREAM_GRAPH_CLASS, offset, key);
        u[0] = r.x; u[1] = r.y; u[2] = r.z; u[3] = r.w;
        a = gd_class_scale(ts[b], B);
    }
    const int gate = user_guided ? pick : 1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (i0 + j >= I) break;
        uint8_t* gp = graph + (int64_t)b * ldg + i0 + j;
        const int c = *gp != 0;
        int s;
        if (sampled) {
            s = sampled[(int64_t)b * lds + i0 + j] != 0;
        } else {
            s = gd_class_draw(c, a, p1_off, u[j]);
        }
        if (sampled_out) sampled_out[(int64_t)b * ldso + i0 + j] = (uint8_t)s;
        *gp = (uint8_t)(c | (s & gate));
    }
}

}  // namespace

extern "C" {

int gdmcf_onehot_noise_f32(const float* x0, int64_t ldx, const int64_t* ts, int B, int I, float discrete,
                           const uint8_t* sampled, int64_t lds, uint64_t seed, uint64_t offset, float* xU, int64_t ldu,
                           uint8_t* sampled_out, int64_t ldso, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && ldx >= I && ldu >= 2 * (int64_t)I, "onehot_noise: bad shape");
    GD_CHECK_OFFSET(offset, "onehot_noise");
    GD_CHECK_ARG(x0 && xU && (sampled ? lds >= I : ts != nullptr) && (!sampled_out || ldso >= I),
                 "onehot_noise: null pointer / bad leading dimension");
    {
        // algorithmic bytes: read x0 (+ the given classes), write the [B, 2I] image
        GdProfScope prof(10, (double)B * I * (4.0 + 8.0 + (sampled ? 1.0 : 0.0)), (hipStream_t)stream);
        hipLaunchKernelGGL(onehot_noise_kernel, dim3(gd_cdiv(I, 1024), B), dim3(256), 0, (hipStream_t)stream, x0, ldx, ts, B,
                           I, gd_p1_off(discrete), sampled, lds, seed, offset, xU, ldu, sampled_out, ldso);
    }
    return gd_launch_status("onehot_noise");
}

int gdmcf_randn_f32(float* out, int64_t ld, int rows, int cols, int stream_id, uint64_t seed, uint64_t offset, void* stream) {
    GD_CHECK_SHAPE(rows > 0 && cols > 0 && ld >= cols, "randn: bad shape");
    GD_CHECK_OFFSET(offset, "randn");
    GD_CHECK_ARG(out && stream_id >= 0 && stream_id < 256, "randn: null pointer / bad stream id");
    {
        GdProfScope prof(11, (double)rows * cols * 4.0, (hipStream_t)stream);  // algorithmic bytes: the store
        hipLaunchKernelGGL(randn_kernel, dim3(gd_cdiv(cols, 256 * PREP_G * 4), rows), dim3(256), 0, (hipStream_t)stream, out,
                           ld, rows, cols, (uint32_t)stream_id, seed, offset);
    }
    return gd_launch_status("randn");
}

int gdmcf_eps_target_f32(const float* noise, int64_t ldn, const float* xt, int64_t ldxt, const float* x0, int64_t ldx0,
                         const int64_t* ts, const float* r1, const float* r2, int t0_likelihood, int B, int I, float* target,
                         int64_t ldt, float* alpha, float* rowdiv, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && ldn >= I && ldxt >= I && ldx0 >= I && ldt >= I, "eps_target: bad shape");
    GD_CHECK_ARG(noise && xt && x0 && ts && r1 && r2 && target && alpha && rowdiv, "eps_target: null pointer");
    GD_CHECK_ARG(target != noise || ldt == ldn, "eps_target: in-place target needs the noise buffer's leading dimension");
    hipLaunchKernelGGL(eps_target_kernel, dim3(gd_cdiv(I, 2048), B), dim3(256), 0, (hipStream_t)stream, noise, ldn, xt, ldxt, x0,
                       ldx0, ts, r1, r2, t0_likelihood, I, target, ldt, alpha, rowdiv);
    return gd_launch_status("eps_target");
}

int gdmcf_graph_guided_step_u8(uint8_t* graph, int64_t ldg, const int64_t* ts, int B, int I, float discrete,
                               const uint8_t* sampled_in, int64_t lds, const uint8_t* pick_in, const float* degree_prob,
                               int user_guided, uint64_t seed, uint64_t offset, uint8_t* sampled_out, int64_t ldso,
                               uint8_t* pick_out, void* stream) {
    GD_CHECK_SHAPE(B > 0 && I > 0 && ldg >= I, "graph_guided_step: bad shape");
    GD_CHECK_OFFSET(offset, "graph_guided_step");
    GD_CHECK_ARG(graph && (sampled_in ? lds >= I : ts != nullptr) && (!sampled_out || ldso >= I),
                 "graph_guided_step: null pointer / bad leading dimension");
    GD_CHECK_ARG(!user_guided || pick_in || degree_prob, "graph_guided_step: user_guided needs pick_in or degree_prob");
    hipLaunchKernelGGL(graph_step_kernel, dim3(gd_cdiv(I, 1024), B), dim3(256), 0, (hipStream_t)stream, graph, ldg, ts, B, I,
                       gd_p1_off(discrete), sampled_in, lds, pick_in, degree_prob, user_guided, seed, offset, sampled_out, ldso, pick_out);
    return gd_launch_status("graph_guided_step");
}

}  // extern "C"
