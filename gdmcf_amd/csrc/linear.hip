// C-ABI entry points for the denoiser's dense layers: forward (plain / fused row-loss / fused
// posterior mean) and backward (input grad, weight grad).  All of them drive gd_gemm_launch (gemm_f32.hip).
//   pick_class, pick_class_dw, pick_splits   the tile class and the K splits of a product
//   Product                                  a product as the kernels take it (GdGemm): the only place that describes one
//   slab_plan, slab_product                  a product as split-K slabs + reducer; gdmcf_linear_ws_bytes sizes from the same plan
//   loss_product, dw_product, BiasCol        what the two loss entries / the three weight-gradient entries share
//   extern "C"                               the entries: argument checks, then the above
#include "common.h"
#include "tail_job.h"

int gd_splitk_reduce(const float* slabs, int64_t slab_stride, int splits, int64_t ld_slab, int M, int N, int mode,
                     const float* bias, const float* rowscale, const float* aact, int64_t ldact, int act, float* out,
                     int64_t ldo, hipStream_t s);  // also refreshes the bf16 shadow of `out`, if one is registered
int gd_colsum(const float* dZ, int64_t ld, const float* rs, int M, int N, float* db, hipStream_t s);
int gd_rowpart_reduce(const float* rowpart, int ld, int M, int nt, float* rowsum, hipStream_t s);

namespace {

// workgroups aimed at by the split-K heuristic: 256 CUs x 2 resident, times ~1.5 so the second wave of
// workgroups evens out the tail (measured sweet spot on the batch-400 products; GDMCF_TARGET_WGS overrides)
static const int TARGET_WGS = gd_env_int("GDMCF_TARGET_WGS", 760);

// input precision of the dense products issued by the calling thread (gdmcf_gemm_precision)
thread_local int t_gemm_prec = GDMCF_GEMM_F32;
// partial row sums per row of the calling thread's last fused-loss product (gdmcf_loss_parts_last)
thread_local int t_loss_parts = 0;

// tile class of an [M,N] output.  bf16 products are bound by L2 reads of the f32 sources, so batch-sized M takes
// the 208x256 class when that wastes little: <= 10 % row padding and, for products that cannot split K
// (`fused`: the epilogue needs complete sums), a last round of workgroups that is mostly full (one 120 KB-LDS
// workgroup per CU).
int pick_class(int M, int N, bool fused, int prec) {
    if (prec == GDMCF_GEMM_BF16 && M > 128) {
        const long pad = (long)gd_cdiv(M, 208) * 208;
        const long tiles = (pad / 208) * gd_cdiv(N, 256);
        const long rounds = (tiles + 255) / 256;
        if (pad * 10 <= (long)M * 11 && pad / 208 <= 2 && (!fused || tiles * 100 >= rounds * 256 * 85)) return 3;
    }
    // three-term split: 2.67x the matrix-pipe rate needs ~40 FLOP per operand byte from L2 -- batch-sized M takes 208-row
    // tiles (208x128: 39.6 FLOP/B against 24.6 at 80x128), one 129 KB-LDS workgroup per CU
    if (prec == GDMCF_GEMM_F32X3 && M > 128 && N >= 128) {
        const long pad = (long)gd_cdiv(M, 208) * 208;
        if (pad * 10 <= (long)M * 11) return 4;
    }
    return gd_pick_shape_class(M, N);
}

// weight-gradient products ([N_out x K_in] outputs, reduction over the batch): bf16 takes the 208x256 class when
// both dimensions are large and the last round of workgroups is mostly full (measured 0.397 -> 0.374 ms on the
// Amazon-Book shape; the kernel is bound by getting the f32 operands through L1, not by MFMA).
int pick_class_dw(int M, int N, int prec, bool fused_adamw = false) {
    static const int forced = gd_env_int("GDMCF_BF16_DW_CLASS", -1);  // tuning knob
    if (prec == GDMCF_GEMM_BF16 && forced >= 0) return forced;
    // AdamW in the epilogue: the kernel is its optimiser stream (26 B per parameter) plus a short, latency-bound k loop that
    // nothing overlaps when one 208x256 workgroup owns the CU: three 80x128 workgroups per CU run one's k loop under the
    // others' streams (Amazon-Book shape, tools/bf16_fused_ablate.sh: 0.61 -> 0.55 ms per weight; 128x128: 0.59)
    if (prec == GDMCF_GEMM_BF16 && fused_adamw && M >= 160 && N >= 256) return 0;
    if (prec == GDMCF_GEMM_BF16 && M >= 416 && N >= 512) {
        const long tiles = (long)gd_cdiv(M, 208) * gd_cdiv(N, 256);
        const long rounds = (tiles + 255) / 256;
        if (tiles * 100 >= rounds * 256 * 85) return 3;
    }
    return gd_pick_shape_class(M, N);
}

// number of K splits for an [M,N,K] product whose output is small (batch x hidden)
int pick_splits(int M, int N, int K, int cls, int prec) {
    const int bk = prec == GDMCF_GEMM_BF16 ? 64 : 32;
    const int tiles = gd_cdiv(M, gd_gemm_tile_m(cls)) * gd_cdiv(N, gd_gemm_tile_n(cls));
    int s = (cls >= 3 ? 256 : TARGET_WGS) / tiles;  // classes 3 and 4: one workgroup per CU
    const int max_by_k = K / (8 * bk);  // keep >= 8 K-tiles per split
    if (s > max_by_k) s = max_by_k;
    if (s < 1) s = 1;
    if (s > 64) s = 64;
    return s;
}

inline int64_t round4(int64_t x) { return (x + 3) & ~(int64_t)3; }

// The product C[M, N] = A B over a reduction of K in the calling thread's precision, operand X stored [rows][K] for layX ==
// GD_LAY_KC and [K][rows] for GD_LAY_MC: the operands, the dimensions, one split, the tile order of class `cls` (the shorter grid
// axis runs fastest) and the profiler tag, written here and nowhere else.  The entry adds what its epilogue reads to `g`.
struct Product {
    GdGemm g = {};
    int layA, layB, cls;

    Product(int layA_, int layB_, const float* A, int64_t lda, const float* B, int64_t ldb, int M, int N, int K, int cls_, int tag)
        : layA(layA_), layB(layB_), cls(cls_) {
        g.bf16 = t_gemm_prec;  // 0 f32, 1 bf16, 2 three-term split
        g.A = A; g.lda = lda; g.B = B; g.ldb = ldb; g.M = M; g.N = N; g.K = K; g.splits = 1;
        g.m_fastest = gd_cdiv(M, gd_gemm_tile_m(cls)) <= gd_cdiv(N, gd_gemm_tile_n(cls));
        g.prof_tag = tag;
        // bf16 mode: stream the operands from their registered bf16 shadows when both have one of exactly this shape
        GdShadow a, b;
        if (g.bf16 != 1 || !gd_shadow_lookup(A, &a) || !gd_shadow_lookup(B, &b)) return;
        const bool okA = layA == GD_LAY_KC ? (a.rows == M && a.cols == K) : (a.rows == K && a.cols == M);
        const bool okB = layB == GD_LAY_KC ? (b.rows == N && b.cols == K) : (b.rows == K && b.cols == N);
        if (!okA || !okB) return;
        g.A16 = a.p16; g.lda16 = a.ld16;
        g.B16 = b.p16; g.ldb16 = b.ld16;
    }

    // the result as an epilogue writes it in place (not split-K slabs): in bf16 mode the kernel keeps C's bf16 shadow in sync
    void result(float* C, int64_t ldc) {
        g.C = C; g.ldc = ldc;
        GdShadow c;
        if (g.bf16 == 1 && gd_shadow_lookup(C, &c) && c.rows == g.M && c.cols >= g.N) {  // x_next lands in a wider xin buffer
            g.C16 = c.p16;
            g.ldc16 = c.ld16;
        }
    }

    int launch(int epi, hipStream_t s) { return gd_gemm_launch(layA, layB, epi, cls, g, s); }
};

// ---- split-K slabs --------------------------------------------------------------------------------------------------------
// An [M, N] product whose output is small against its reduction: `splits` partial products over K ranges into slabs
// [splits][M][ld] of the caller's workspace, summed by gd_splitk_reduce with the layer's bias / activation / row scale.
struct SlabPlan {
    int cls, splits;
    int64_t ld;
};
SlabPlan slab_plan(int M, int N, int K, int prec) {
    const int cls = pick_class(M, N, false, prec);
    return {cls, pick_splits(M, N, K, cls, prec), round4(N)};
}

// what gd_splitk_reduce does with the sum (mode 0: bias + activation, the forward; 1: row scale and the activation's derivative)
struct SlabReduce {
    int mode;
    const float* bias;
    const float* rowscale;
    const float* aact;
    int64_t ldact;
    int act;
    float* out;
    int64_t ldo;
};

// p as slabs in ws, then the reducer.  The kernel that takes the product may split further than the plan when ws_cap allows
// (gdmcf_linear_ws_bytes sizes for it) and says so in g.kchunk.  job: a tail job that has to ride the launch, which only
// dr_kn_kernel offers -- GD_DR_NOT_TAKEN and nothing launched where it does not take both.
int slab_product(Product& p, const SlabPlan& plan, const char* who, void* ws, size_t ws_bytes, const GdTailJob* job,
                 const SlabReduce& r, hipStream_t s) {
    GdGemm& g = p.g;
    const size_t need = (size_t)plan.splits * g.M * plan.ld * sizeof(float);
    if (job) {
        if (ws == nullptr) return GD_DR_NOT_TAKEN;  // (the kernel checks ws_cap against its own split count)
    } else if (ws == nullptr || ws_bytes < need) {
        gdmcf_set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, need);
        return GDMCF_E_WORKSPACE;
    }
    g.splits = plan.splits; g.C = (float*)ws; g.ldc = plan.ld; g.slab_stride = (int64_t)g.M * plan.ld;
    g.ws_cap = ws_bytes;
    const int rc = job ? gd_dr_kn_launch_tail(g, *job, s) : p.launch(GD_EPI_SLAB, s);
    if (rc) return rc;
    return gd_splitk_reduce((const float*)ws, g.slab_stride, gd_cdiv(g.K, g.kchunk), plan.ld, g.M, g.N, r.mode, r.bias, r.rowscale,
                            r.aact, r.ldact, r.act, r.out, r.ldo, s);
}

// floats of slab workspace an [M, N, K] product may use in precision prec: the plan's, or in float32 what the direct-to-register
// kernel that takes it would split into (dr_kn_kernel: the input gradient and gdmcf_linear_fwd_wt_f32; fat: also the fat-tile slab
// loop, the forward only)
size_t slab_floats(int M, int N, int K, int prec, bool fat) {
    const SlabPlan plan = slab_plan(M, N, K, prec);
    int splits = plan.splits;
    if (prec == GDMCF_GEMM_F32) {
        const int kn = gd_dr_kn_splits(M, N, K), ft = fat ? gd_dr_fat_slab_plan(M, N, K, nullptr, nullptr) : 0;
        splits = splits > kn ? splits : kn;
        splits = splits > ft ? splits : ft;
    }
    return (size_t)splits * M * plan.ld;
}

// ---- the fused row loss ---------------------------------------------------------------------------------------------------
// diff = alpha . (A W^T + bias) - target with its row sums of squares, the target as floats or as a bitmap of {0, 1} rows
int loss_product(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, const float* target, int64_t ldt,
                 const uint32_t* target_bits, int64_t ldbits, const float* alpha, int M, int N, int K, float* out, int64_t ldo,
                 float* diff, int64_t ldd, float* rowpart, float* rowsum, hipStream_t s) {
    Product p(GD_LAY_KC, GD_LAY_KC, A, lda, W, ldw, M, N, K, pick_class(M, N, true, t_gemm_prec), 2);
    GdGemm& g = p.g;
    g.bias = bias; g.aux = target; g.ldaux = ldt; g.aux_bits = target_bits; g.ldbits = ldbits; g.r0 = alpha;
    g.out2 = out; g.ldout2 = ldo; g.rowpart = rowpart; g.ld_rowpart = gdmcf_loss_tiles(N);
    p.result(diff, ldd);
    int rc = p.launch(GD_EPI_LOSS, s);
    if (rc) return rc;
    t_loss_parts = g.tiles_n;
    if (rowsum == nullptr) return GDMCF_OK;  // the caller reduces (gdmcf_linear_bwd_input_tail_f32)
    return gd_rowpart_reduce(rowpart, g.ld_rowpart, M, g.tiles_n, rowsum, s);
}

// ---- weight gradients -----------------------------------------------------------------------------------------------------
// dW[N x K_in] = dZ[M x N]^T A[M x K_in] -> gemm (N, K, reduction M), both operands row-contiguous
Product dw_product(const float* dZ, int64_t lddz, const float* A, int64_t lda, int M, int N, int K, bool fused_adamw) {
    return Product(GD_LAY_MC, GD_LAY_MC, dZ, lddz, A, lda, N, K, M, pick_class_dw(N, K, t_gemm_prec, fused_adamw), 5);
}

// The bias gradient db[n] = sum_m rowscale[m] dZ[m, n] as column K of the weight-gradient product p: possible when the caller
// states (a_scale_col) that column K of the activation operand A holds rowscale[m] -- gdmcf_rowscale_f32 writes it there when its
// output has room (ldo > K).  Nothing is remembered between calls.  The request is GdGemm::out2 = db; a launcher that takes it
// clears the field, and finish() runs the column sum where the product did not deliver.
struct BiasCol {
    const float* dZ = nullptr;
    int64_t lddz = 0;
    const float* rowscale = nullptr;
    int M = 0, N = 0;
    float* db = nullptr;
    bool asked = false;

    BiasCol() = default;
    BiasCol(GdGemm& g, int a_scale_col, const float* rowscale_, float* db_)
        : dZ(g.A), lddz(g.lda), rowscale(rowscale_), M(g.K), N(g.M), db(db_) {
        static const int on = gd_env_int("GDMCF_BIAS_COL", 1);
        asked = on && a_scale_col && db != nullptr && t_gemm_prec == GDMCF_GEMM_F32 && g.ldb > g.N;
        g.out2 = asked ? db : nullptr;
    }
    int finish(const GdGemm& g, hipStream_t s) const {
        if (asked && g.out2 == nullptr) return GDMCF_OK;  // db came out of the product
        return db ? gd_colsum(dZ, lddz, rowscale, M, N, db, s) : GDMCF_OK;
    }
};

int dw_adamw_check(const GdDwAdamw& e) {
    GD_CHECK_SHAPE(e.M > 0 && e.N > 0 && e.K > 0 && e.lddz >= e.N && e.lda >= e.K && e.ldw >= e.K, "linear_bwd_weight_adamw: bad shape");
    GD_CHECK_ARG(e.W && e.exp_avg && e.exp_avg_sq && e.step >= 1, "linear_bwd_weight_adamw: optimizer state missing");
    return GDMCF_OK;
}

// The product of one (checked) fused weight-gradient + AdamW call: W / exp_avg / exp_avg_sq updated in its epilogue, which in
// the bf16 kernels also refreshes W's bf16 shadow
Product dw_adamw_product(const GdDwAdamw& e, BiasCol& col) {
    Product p = dw_product(e.dZ, e.lddz, e.A, e.lda, e.M, e.N, e.K, true);
    p.result(e.W, e.ldw);
    p.g.aux = e.exp_avg; p.g.aux2 = e.exp_avg_sq;
    p.g.adam = gd_adam_hyper(e.lr, e.beta1, e.beta2, e.eps, e.weight_decay, e.step, e.grad_scale);
    p.g.adam_dev = t_gd_step_state ? &t_gd_step_state->hyper : nullptr;  // bound graph step state: the scalars of the step being replayed
    col = BiasCol(p.g, e.a_scale_col, e.rowscale, e.db);
    return p;
}

}  // namespace

extern "C" {

int gdmcf_gemm_precision(int mode) {
    const int prev = t_gemm_prec;
    if (mode == GDMCF_GEMM_F32 || mode == GDMCF_GEMM_BF16 || mode == GDMCF_GEMM_F32X3) t_gemm_prec = mode;
    return prev;
}

size_t gdmcf_linear_ws_bytes(int M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    // forward: slabs [splits][M][round4(N)];  backward-input: slabs [splits][M][round4(K)]
    size_t need = 0;
    for (int prec = GDMCF_GEMM_F32; prec <= GDMCF_GEMM_F32X3; ++prec) {  // the caller may switch precision later
        const size_t f = slab_floats(M, N, K, prec, true), b = slab_floats(M, K, N, prec, false);
        need = need > f ? need : f;
        need = need > b ? need : b;
    }
    return need * sizeof(float) + 256;
}

int gdmcf_debug_fat_slab_plan(int M, int N, int K, int* nb, int* splits, int* cps) {
    int nb_ = 0, cps_ = 0;
    const int sp = (t_gemm_prec == GDMCF_GEMM_F32 && M > 0 && N > 0 && K > 0) ? gd_dr_fat_slab_plan(M, N, K, &nb_, &cps_) : 0;
    if (nb) *nb = nb_;
    if (splits) *splits = sp;
    if (cps) *cps = cps_;
    return sp > 0;
}

int gdmcf_loss_tiles(int N) { return gd_cdiv(N, 16); }  // partial row sums per output tile: the narrowest tile any kernel uses

int gdmcf_linear_fwd_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias, int act, int M,
                         int N, int K, float* C, int64_t ldc, void* ws, size_t ws_bytes, void* stream) {
    GD_CHECK_SHAPE(M > 0 && N > 0 && K > 0 && lda >= K && ldw >= K && ldc >= N, "linear_fwd: bad shape");
    GD_CHECK_ARG(act == 0 || act == 1, "linear_fwd: bad activation");
    hipStream_t s = (hipStream_t)stream;
    const SlabPlan plan = slab_plan(M, N, K, t_gemm_prec);
    Product p(GD_LAY_KC, GD_LAY_KC, A, lda, W, ldw, M, N, K, plan.cls, 1);
    p.g.bias = bias; p.g.act = act;
    if (plan.splits == 1) {
        p.result(C, ldc);
        return p.launch(GD_EPI_BIAS_ACT, s);
    }
    return slab_product(p, plan, "linear_fwd", ws, ws_bytes, nullptr, {0, bias, nullptr, nullptr, 0, act, C, ldc}, s);
}

int gdmcf_linear_fwd_wt_f32(const float* A, int64_t lda, const float* Wt, int64_t ldwt, const float* bias, int act, int M, int N,
                            int K, float* C, int64_t ldc, void* ws, size_t ws_bytes, void* stream) {
    GD_CHECK_SHAPE(M > 0 && N > 0 && K > 0 && lda >= K && ldwt >= N && ldc >= N, "linear_fwd_wt: bad shape");
    GD_CHECK_ARG(act == 0 || act == 1, "linear_fwd_wt: bad activation");
    if (t_gemm_prec != GDMCF_GEMM_F32) {
        gdmcf_set_error("linear_fwd_wt: float32 GEMM mode only (the bf16 / f32x3 modes keep the weight in its own orientation)");
        return GDMCF_E_UNSUPPORTED;
    }
    // the product of the input gradient, with a forward reducer: [M x N] = A[M x K] * Wt[K x N], split over K
    const SlabPlan plan = slab_plan(M, N, K, t_gemm_prec);
    Product p(GD_LAY_KC, GD_LAY_MC, A, lda, Wt, ldwt, M, N, K, plan.cls, 1);
    return slab_product(p, plan, "linear_fwd_wt", ws, ws_bytes, nullptr, {0, bias, nullptr, nullptr, 0, act, C, ldc}, (hipStream_t)stream);
}

int gdmcf_linear_loss_fwd_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                              const float* target, int64_t ldt, const float* alpha, int M, int N, int K, float* out,
                              int64_t ldo, float* diff, int64_t ldd, float* rowpart, float* rowsum, void* stream) {
    GD_CHECK_SHAPE(M > 0 && N > 0 && K > 0 && lda >= K && ldw >= K && ldt >= N && ldd >= N, "linear_loss_fwd: bad shape");
    GD_CHECK_SHAPE(out == nullptr || ldo >= N, "linear_loss_fwd: ldo < N");
    return loss_product(A, lda, W, ldw, bias, target, ldt, nullptr, 0, alpha, M, N, K, out, ldo, diff, ldd, rowpart, rowsum,
                        (hipStream_t)stream);
}

int gdmcf_linear_loss_fwd_bits_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                                   const uint32_t* target_bits, int64_t ldbits, const float* alpha, int M, int N, int K,
                                   float* out, int64_t ldo, float* diff, int64_t ldd, float* rowpart, float* rowsum,
                                   void* stream) {
    GD_CHECK_SHAPE(M > 0 && N > 0 && K > 0 && lda >= K && ldw >= K && ldd >= N, "linear_loss_fwd_bits: bad shape");
    GD_CHECK_SHAPE(out == nullptr || ldo >= N, "linear_loss_fwd_bits: ldo < N");
    GD_CHECK_ARG(target_bits && ldbits >= (N + 31) / 32, "linear_loss_fwd_bits: target bitmap missing / ldbits < ceil(N/32)");
    return loss_product(A, lda, W, ldw, bias, nullptr, 0, target_bits, ldbits, alpha, M, N, K, out, ldo, diff, ldd, rowpart, rowsum,
                        (hipStream_t)stream);
}

int gdmcf_linear_posterior_fwd_f32(const float* A, int64_t lda, const float* W, int64_t ldw, const float* bias,
                                   const float* x_t, int64_t ldxt, const float* c1, const float* c2, const float* r1,
                                   const float* r2, const float* sigma, const float* z, int64_t ldz, int M, int N,
                                   int K, float* x_next, int64_t ldxn, float* pred_out, int64_t ldp, void* stream) {
    GD_CHECK_SHAPE(M > 0 && N > 0 && K > 0 && lda >= K && ldw >= K && ldxt >= N && ldxn >= N, "linear_posterior_fwd: bad shape");
    GD_CHECK_ARG(c1 && c2, "linear_posterior_fwd: c1/c2 missing");
    GD_CHECK_ARG((r1 == nullptr) == (r2 == nullptr), "linear_posterior_fwd: r1/r2 must both be set or both NULL");
    GD_CHECK_ARG(z == nullptr || (sigma != nullptr && ldz >= N), "linear_posterior_fwd: sigma missing");
    Product p(GD_LAY_KC, GD_LAY_KC, A, lda, W, ldw, M, N, K, pick_class(M, N, true, t_gemm_prec), 3);
    GdGemm& g = p.g;
    g.bias = bias; g.aux = x_t; g.ldaux = ldxt; g.aux2 = z; g.ldaux2 = ldz;
    g.r0 = c1; g.r1 = c2; g.r2 = r1; g.r3 = r2; g.r4 = sigma;
    g.out2 = pred_out; g.ldout2 = ldp;
    p.result(x_next, ldxn);
    return p.launch(GD_EPI_POST, (hipStream_t)stream);
}

// product dims: [M x K_in] = dZ[M x N] * W[N x K_in]  -> gemm (M, K, reduction N); job: slab_product
static int bwd_input(const char* who, const float* dZ, int64_t lddz, const float* W, int64_t ldw, const float* rowscale,
                     const float* Aact, int64_t ldact, int act, int M, int N, int K, float* dA, int64_t ldda, void* ws,
                     size_t ws_bytes, const GdTailJob* job, hipStream_t s) {
    const SlabPlan plan = slab_plan(M, K, N, t_gemm_prec);
    Product p(GD_LAY_KC, GD_LAY_MC, dZ, lddz, W, ldw, M, K, N, plan.cls, 4);
    return slab_product(p, plan, who, ws, ws_bytes, job, {1, nullptr, rowscale, Aact, ldact, act, dA, ldda}, s);
}

int gdmcf_linear_bwd_input_f32(const float* dZ, int64_t lddz, const float* W, int64_t ldw, const float* rowscale,
                               const float* Aact, int64_t ldact, int act, int M, int N, int K, float* dA,
                               int64_t ldda, void* ws, size_t ws_bytes, void* stream) {
    GD_CHECK_SHAPE(M > 0 && N > 0 && K > 0 && lddz >= N && ldw >= K && ldda >= K, "linear_bwd_input: bad shape");
    GD_CHECK_ARG(act == 0 || (act == 1 && Aact && ldact >= K), "linear_bwd_input: activation output missing");
    return bwd_input("linear_bwd_input", dZ, lddz, W, ldw, rowscale, Aact, ldact, act, M, N, K, dA, ldda, ws, ws_bytes, nullptr,
                     (hipStream_t)stream);
}

int gdmcf_loss_parts_last(void) { return t_loss_parts; }

int gdmcf_kn_tail_run(const GdKnTail* tail, int M, void* stream) {
    GD_CHECK_ARG(tail != nullptr, "kn_tail_run: tail missing");
    const GdKnTail& t = *tail;
    GD_CHECK_SHAPE(M > 0 && t.nt > 0 && t.ld_rowpart >= t.nt, "kn_tail_run: bad shape");
    GD_CHECK_ARG(t.rowpart && t.rowsum, "kn_tail_run: null pointer");
    int rc = gd_rowpart_reduce(t.rowpart, t.ld_rowpart, M, t.nt, t.rowsum, (hipStream_t)stream);
    if (rc) return rc;
    rc = gdmcf_row_loss_finish_mean_f64(t.rowsum, t.rowdiv, t.alpha, t.ts, t.weight_t, t.pt, M, t.T, t.H, t.Lt_history, t.Lt_count,
                                        t.update_history, t.loss_unscaled, t.loss, t.gradcoef, t.loss_mean, t.rowscale_mean, stream);
    if (rc) return rc;
    return gdmcf_rowscale_f32(t.A, t.lda, t.rowscale, M, t.Ka, t.out, t.ldo, stream);
}

int gdmcf_linear_bwd_input_tail_f32(const float* dZ, int64_t lddz, const float* W, int64_t ldw, const float* rowscale,
                                    const float* Aact, int64_t ldact, int act, int M, int N, int K, float* dA, int64_t ldda,
                                    void* ws, size_t ws_bytes, const GdKnTail* tail, void* stream) {
    GD_CHECK_SHAPE(M > 0 && N > 0 && K > 0 && lddz >= N && ldw >= K && ldda >= K, "linear_bwd_input_tail: bad shape");
    GD_CHECK_ARG(act == 0 || (act == 1 && Aact && ldact >= K), "linear_bwd_input_tail: activation output missing");
    GD_CHECK_ARG(tail != nullptr, "linear_bwd_input_tail: tail missing");
    const GdKnTail& t = *tail;
    // (the three launches' own checks, ahead of anything launched)
    GD_CHECK_SHAPE(t.nt > 0 && t.ld_rowpart >= t.nt && t.T > 0 && t.H > 0 && t.Ka > 0 && t.lda >= t.Ka && t.ldo >= t.Ka,
                   "linear_bwd_input_tail: bad tail shape");
    GD_CHECK_ARG(t.rowpart && t.rowsum && t.rowdiv && t.ts && t.weight_t && t.pt && t.loss_unscaled && t.loss && t.A && t.rowscale && t.out,
                 "linear_bwd_input_tail: null pointer");
    GD_CHECK_ARG(!t.update_history || (t.Lt_history && t.Lt_count), "linear_bwd_input_tail: update_history without the history");
    GD_CHECK_ARG(!t.rowscale_mean || t.gradcoef, "linear_bwd_input_tail: rowscale_mean needs gradcoef");
    GD_CHECK_ARG(lt_lds_bytes(t.T, t.H, M) <= GD_LT_LDS_MAX, "linear_bwd_input_tail: T*H and B too large for the LDS-resident FIFO update (150 KiB)");
    hipStream_t s = (hipStream_t)stream;
    if (t_gemm_prec == GDMCF_GEMM_F32) {  // the input gradient on dr_kn_kernel with the tail on its idle workgroup
        GdShadow sh;
        const bool has16 = gd_shadow_lookup(t.out, &sh) && sh.rows == M && sh.cols == t.Ka;  // as gdmcf_rowscale_f32
        GdTailJob j = {};
        j.on = 1; j.B = M;
        j.rowpart = t.rowpart; j.ld_rowpart = t.ld_rowpart; j.nt = t.nt; j.rowsum = t.rowsum;
        j.rowdiv = t.rowdiv; j.alpha = t.alpha; j.gradcoef = t.gradcoef; j.ts = t.ts; j.weight_t = t.weight_t; j.pt = t.pt;
        j.T = t.T; j.H = t.H; j.update = t.update_history; j.hist = t.Lt_history; j.cnt = t.Lt_count; j.lu = t.loss_unscaled;
        j.loss = t.loss; j.loss_mean = t.loss_mean; j.rowscale_mean = t.rowscale_mean; j.inv_b = 1.0f / (float)M;
        j.K = t.Ka; j.A = t.A; j.lda = t.lda; j.rs = t.rowscale; j.out = t.out; j.ldo = t.ldo;
        j.out16 = has16 ? (unsigned short*)sh.p16 : nullptr; j.ldo16 = has16 ? sh.ld16 : 0; j.bias_col = t.ldo > t.Ka;
        const int rc = bwd_input("linear_bwd_input_tail", dZ, lddz, W, ldw, rowscale, Aact, ldact, act, M, N, K, dA, ldda, ws, ws_bytes, &j, s);
        if (rc != GD_DR_NOT_TAKEN) return rc;
    }
    const int rc = gdmcf_kn_tail_run(tail, M, stream);
    if (rc) return rc;
    return gdmcf_linear_bwd_input_f32(dZ, lddz, W, ldw, rowscale, Aact, ldact, act, M, N, K, dA, ldda, ws, ws_bytes, stream);
}

int gdmcf_linear_bwd_weight_f32(const float* dZ, int64_t lddz, const float* A, int64_t lda, const float* rowscale,
                                int a_scale_col, int M, int N, int K, float* dW, int64_t lddw, float* db, int accumulate,
                                void* stream) {
    GD_CHECK_SHAPE(M > 0 && N > 0 && K > 0 && lddz >= N && lda >= K && lddw >= K, "linear_bwd_weight: bad shape");
    hipStream_t s = (hipStream_t)stream;
    Product p = dw_product(dZ, lddz, A, lda, M, N, K, false);
    p.g.C = dW; p.g.ldc = lddw; p.g.accumulate = accumulate;  // (not result(): a gradient keeps no bf16 shadow)
    const BiasCol col(p.g, a_scale_col, rowscale, db);
    const int rc = p.launch(GD_EPI_STORE, s);
    return rc ? rc : col.finish(p.g, s);
}

int gdmcf_linear_bwd_weight_adamw_f32(const float* dZ, int64_t lddz, const float* A, int64_t lda, const float* rowscale,
                                      int a_scale_col, int M, int N, int K, float* W, int64_t ldw, float* exp_avg, float* exp_avg_sq,
                                      float* db, float lr, float beta1, float beta2, float eps, float weight_decay,
                                      int step, float grad_scale, void* stream) {
    const GdDwAdamw e = {dZ, lddz, A, lda, rowscale, a_scale_col, M, N, K, W, ldw, exp_avg, exp_avg_sq, db,
                         lr, beta1, beta2, eps, weight_decay, step, grad_scale};
    int rc = dw_adamw_check(e);
    if (rc) return rc;
    BiasCol col;
    Product p = dw_adamw_product(e, col);
    rc = p.launch(GD_EPI_ADAMW, (hipStream_t)stream);
    return rc ? rc : col.finish(p.g, (hipStream_t)stream);
}

int gdmcf_linear_bwd_weight_adamw_multi_f32(const GdDwAdamw* list, int n, void* stream) {
    GD_CHECK_ARG(n >= 0 && (n == 0 || list), "linear_bwd_weight_adamw_multi: bad list");
    hipStream_t s = (hipStream_t)stream;
    constexpr int MAXN = 4;  // products per launch (gemm_dr_tn.hip: DR_MULTI_MAX)
    for (int i0 = 0; i0 < n; i0 += MAXN) {
        const int k = n - i0 < MAXN ? n - i0 : MAXN;
        GdGemm g[MAXN];
        BiasCol col[MAXN];
        for (int j = 0; j < k; ++j) {
            const int rc = dw_adamw_check(list[i0 + j]);
            if (rc) return rc;
            g[j] = dw_adamw_product(list[i0 + j], col[j]).g;
        }
        int rc = gd_gemm_dr_adamw_multi(g, k, s);
        if (rc == GD_DR_NOT_TAKEN) {  // one call per product
            for (int j = 0; j < k; ++j) {
                const GdDwAdamw& e = list[i0 + j];
                rc = gdmcf_linear_bwd_weight_adamw_f32(e.dZ, e.lddz, e.A, e.lda, e.rowscale, e.a_scale_col, e.M, e.N, e.K, e.W,
                                                       e.ldw, e.exp_avg, e.exp_avg_sq, e.db, e.lr, e.beta1, e.beta2, e.eps,
                                                       e.weight_decay, e.step, e.grad_scale, stream);
                if (rc) return rc;
            }
            continue;
        }
        if (rc) return rc;
        for (int j = 0; j < k; ++j) {
            rc = col[j].finish(g[j], s);
            if (rc) return rc;
        }
    }
    return GDMCF_OK;
}

}  // extern "C"
