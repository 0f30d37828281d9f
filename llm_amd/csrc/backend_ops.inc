// backend_ops.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip, inside its anonymous
// namespace where noted): op launchers — activation re-quantization, the quantized mat-vec / GEMM dispatch (incl. the resident f16 weight copies), K-quants, attention products, element-wise ops, get_rows.  Inside the anonymous namespace.
// ---------------------------------------------------------------------------------------------------
// op launchers
// ---------------------------------------------------------------------------------------------------
bool is_contig_f32(const ggml_tensor *t) { return t->type == GGML_TYPE_F32 && ggml_is_contiguous(t); }

// ---- the activation quantizers' launches: grid, block and dynamic LDS of each kernel, one text for the executor, the plans and
// the test hook ggml_hip_debug_act_quant (debug_quant_attn.inc).  Accounting (Timed / cx) stays with the callers.
// 32 lanes per block, rows of nb_row bytes
void launch_quantize_act(bool f16_d, const char *x, int64_t nb_row, int64_t nb, int64_t N, int8_t *lo, int8_t *hi, float *d, int *s) {
    with_bool(f16_d, [&](auto F16D) {
        hipLaunchKernelGGL(k_quantize_act<CT(F16D)>, grid1(nb * N * 32), dim3(256), 0, g.stream, x, nb_row, nb, N, lo, hi, d, s);
    });
}
void launch_quant_act_f16(bool f16_d, const char *x, int64_t nb_row, int64_t nb, int64_t N, _Float16 *out) {
    with_bool(f16_d, [&](auto F16D) {
        hipLaunchKernelGGL(k_quant_act_f16<CT(F16D)>, grid1(nb * N * 32), dim3(256), 0, g.stream, x, nb_row, nb, N, out);
    });
}
void launch_quant_act_i8(bool f16_d, const char *x, int64_t nb_row, int64_t nb, int64_t N, float zp, int8_t *q8, float *dq, float *xs) {
    with_bool(f16_d, [&](auto F16D) {
        hipLaunchKernelGGL(k_quant_act_i8<CT(F16D)>, grid1(nb * N * 32), dim3(256), 0, g.stream, x, nb_row, nb, N, zp, q8, dq, xs);
    });
}
// one workgroup per (super-block, row)
void launch_quant_q8k(const char *x, int64_t nb_row, int64_t nsb, int64_t N, int8_t *q8, float *d8, int16_t *bs) {
    hipLaunchKernelGGL(k_quant_q8k, dim3((unsigned)nsb, (unsigned)N), dim3(256), 0, g.stream, x, nb_row, nsb, q8, d8, bs);
}
void launch_quant_act_f16_k(const char *x, int64_t nb_row, int64_t nsb, int64_t N, _Float16 *out) {
    hipLaunchKernelGGL(k_quant_act_f16_k, dim3((unsigned)nsb, (unsigned)N), dim3(256), 0, g.stream, x, nb_row, nsb, out);
}
void launch_f32_to_w16(const float *src, int64_t n /* elements, a multiple of 32 */, _Float16 *out) {
    hipLaunchKernelGGL(k_f32_to_w16, grid1(n), dim3(256), 0, g.stream, src, n / 32, out);
}
// the plans' planar Q8 rows: blockIdx.y = row; dT / sT (nullable): the [block][8] tables, rows 8p .. 8p + 7 in table p
void launch_quant_row(bool f16_d, const float *x, int64_t nb, int64_t N, int8_t *lo, int8_t *hi, float *d, int *s, float *dT, int *sT) {
    const dim3 grid(grid1(nb * 32).x, (unsigned)N);
    with_bool(f16_d, [&](auto F16D) { hipLaunchKernelGGL(k_quant_row<CT(F16D)>, grid, dim3(256), 0, g.stream, x, (int)nb, lo, hi, d, s, dT, sT); });
}
// one 1024-thread workgroup per row; cw (nullable): the launch on every CU whose other workgroups warm the next launch's rows
void launch_rmsnorm_quant(bool f16_d, const float *x, const float *w, float eps, int64_t E, int64_t N, float *y, int8_t *lo, int8_t *hi,
                          float *d, int *s, float *dT, int *sT, const ColsWarm *cw) {
    with_bool(f16_d, [&](auto F16D) {
        if (cw)
            hipLaunchKernelGGL(k_rmsnorm_quant_warm<CT(F16D)>, dim3((unsigned)g.num_cus), dim3(1024), (size_t)E * 4, g.stream, x, w, eps, (int)E, y,
                               lo, hi, d, s, dT, sT, (int)N, *cw);
        else
            hipLaunchKernelGGL(k_rmsnorm_quant<CT(F16D)>, dim3((unsigned)N), dim3(1024), (size_t)E * 4, g.stream, x, w, eps, (int)E, y, lo, hi, d, s,
                               dT, sT);
    });
}
// the K plan's helpers: Q8_K rows [N][nsb * 256]
void launch_k_norm_quant(const float *x, const float *w, float eps, int64_t E, int64_t N, float *y, int8_t *q8, float *d8, int16_t *bs) {
    hipLaunchKernelGGL(k_k_norm_quant, dim3((unsigned)(E / 256), (unsigned)N), dim3(256), 0, g.stream, x, w, eps, (int)E, y, q8, d8, bs);
}
void launch_k_quant(const float *x, int64_t nsb, int64_t N, int8_t *q8, float *d8, int16_t *bs) {
    hipLaunchKernelGGL(k_k_quant, dim3((unsigned)nsb, (unsigned)N), dim3(256), 0, g.stream, x, q8, d8, bs);
}
void launch_k_silu_mul_quant(const float *g1, const float *g3, int64_t nsb, int64_t N, int8_t *q8, float *d8, int16_t *bs) {
    hipLaunchKernelGGL(k_k_silu_mul_quant, dim3((unsigned)nsb, (unsigned)N), dim3(256), 0, g.stream, g1, g3, q8, d8, bs);
}
// the prompt plan's f16 operands; kq: the Q8_K round trip (a K-quant weight's GEMM), else Q8_0 / Q8_1 by f16_d
void launch_p_norm_quant(bool kq, bool f16_d, const float *x, const float *x2, const float *r, float *xsum, const float *w, float eps,
                         int64_t E, int64_t N, float *y_f32, _Float16 *out) {
    with_bool(r != nullptr, [&](auto RES) {
        if (kq)
            hipLaunchKernelGGL((k_p_norm_quant<false, CT(RES), true>), dim3((unsigned)N), dim3(256), (size_t)E * 4, g.stream, x, x2, r, xsum, w, eps, (int)E, y_f32, out);
        else
            with_bool(f16_d, [&](auto F16D) {
                hipLaunchKernelGGL((k_p_norm_quant<CT(F16D), CT(RES)>), dim3((unsigned)N), dim3(256), (size_t)E * 4, g.stream, x, x2, r, xsum, w, eps, (int)E, y_f32, out);
            });
    });
}
void launch_p_quant4(bool kq, bool f16_d, const f32x4 *a, int64_t n4, _Float16 *out) {
    const dim3 grid((unsigned)((n4 + 255) / 256));
    if (kq)
        hipLaunchKernelGGL((k_p_quant4<false, true>), grid, dim3(256), 0, g.stream, a, n4, out);
    else
        with_bool(f16_d, [&](auto F16D) { hipLaunchKernelGGL(k_p_quant4<CT(F16D)>, grid, dim3(256), 0, g.stream, a, n4, out); });
}
void launch_p_silu_mul_quant(bool kq, bool f16_d, const f32x4 *a, const f32x4 *b, int64_t n4, int64_t part4, _Float16 *out) {
    const dim3 grid((unsigned)((n4 + 255) / 256));
    if (kq)
        hipLaunchKernelGGL((k_p_silu_mul_quant<false, true>), grid, dim3(256), 0, g.stream, a, b, n4, part4, out);
    else
        with_bool(f16_d, [&](auto F16D) { hipLaunchKernelGGL(k_p_silu_mul_quant<CT(F16D)>, grid, dim3(256), 0, g.stream, a, b, n4, part4, out); });
}

QAct quantize_activation(const ggml_tensor *src1, bool f16_d) {
    BK_ASSERT(src1->type == GGML_TYPE_F32 && src1->nb[0] == 4 && src1->ne[2] == 1 && src1->ne[3] == 1);
    const int64_t K = src1->ne[0], N = src1->ne[1], nb = K / 32;
    if (g_qact.valid && g_qact.src_data == src1->data && g_qact.f16_d == f16_d && g_qact.nb == nb && g_qact.ncols == N)
        return g_qact.act;
    const size_t nblk = (size_t)nb * N;
    char *blk = ws_alloc(nblk * 40);
    char *lo = blk, *hi = blk + nblk * 16, *d = blk + nblk * 32, *s = blk + nblk * 36;
    const char *x = dev_ptr(src1);
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)(K * N * 4 + nblk * 40));
    launch_quantize_act(f16_d, x, (int64_t)src1->nb[1], nb, N, (int8_t *)lo, (int8_t *)hi, (float *)d, (int *)s);
    HIP_CHECK(hipGetLastError());
    g_qact.valid = true;
    g_qact.src_data = src1->data;
    g_qact.src_bytes = ggml_nbytes(src1);
    g_qact.f16_d = f16_d;
    g_qact.nb = nb;
    g_qact.ncols = N;
    g_qact.act = QAct{(const i32x4 *)lo, (const i32x4 *)hi, (const float *)d, (const int *)s};
    return g_qact.act;
}

size_t blk_bytes(int qt) { return qt == QT_Q4_0 ? 18 : qt == QT_Q4_1 ? 20 : qt == QT_Q5_0 ? 22 : qt == QT_Q5_1 ? 24 : 34; }

template <int QT, int NCOLS>
void launch_mmvq_r(const MmvqArgs &a, int R, int nwg, size_t lds) {
    switch (R) {
        case 1: hipLaunchKernelGGL((k_mmvq<QT, NCOLS, 1>), dim3(nwg), dim3(256), lds, g.stream, a); break;
        case 2: hipLaunchKernelGGL((k_mmvq<QT, NCOLS, 2>), dim3(nwg), dim3(256), lds, g.stream, a); break;
        default: hipLaunchKernelGGL((k_mmvq<QT, NCOLS, 4>), dim3(nwg), dim3(256), lds, g.stream, a); break;
    }
}
template <int QT>
void launch_mmvq_c(const MmvqArgs &a, int ncols, int R, int nwg, size_t lds) {
    switch (ncols) {
        case 1: launch_mmvq_r<QT, 1>(a, R, nwg, lds); break;
        case 2: launch_mmvq_r<QT, 2>(a, R, nwg, lds); break;
        case 4: launch_mmvq_r<QT, 4>(a, R, nwg, lds); break;
        case 8: launch_mmvq_r<QT, 8>(a, R, nwg, lds); break;
        default: die("mmvq: bad ncols %d", ncols);
    }
}
void launch_mmvq(int qt, const MmvqArgs &a, int ncols, int R, int nwg, size_t lds) {
    with_qt(qt, [&](auto QT) { launch_mmvq_c<CT(QT)>(a, ncols, R, nwg, lds); }, "mmvq: bad weight type");
    HIP_CHECK(hipGetLastError());
}

const _Float16 *quantize_activation_f16(const ggml_tensor *src1, bool f16_d) {
    BK_ASSERT(src1->type == GGML_TYPE_F32 && src1->nb[0] == 4 && src1->ne[2] == 1 && src1->ne[3] == 1);
    const int64_t K = src1->ne[0], N = src1->ne[1], nb = K / 32;
    if (g_xf16.valid && g_xf16.src_data == src1->data && g_xf16.f16_d == f16_d && g_xf16.nb == nb && g_xf16.ncols == N)
        return g_xf16.x;
    _Float16 *out = (_Float16 *)ws_alloc((size_t)N * K * 2);
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)(K * N * 6));
    launch_quant_act_f16(f16_d, dev_ptr(src1), (int64_t)src1->nb[1], nb, N, out);
    HIP_CHECK(hipGetLastError());
    g_xf16.valid = true;
    g_xf16.src_data = src1->data;
    g_xf16.src_bytes = ggml_nbytes(src1);
    g_xf16.f16_d = f16_d;
    g_xf16.nb = nb;
    g_xf16.ncols = N;
    g_xf16.x = out;
    return out;
}

struct XI8Buf {  // int8 activations + f32 block scale + zero-point term of the integer prompt GEMM (kernels/mmq_i8.h)
    const void *src_data = nullptr;
    size_t src_bytes = 0;
    int qt = -1;
    int64_t nb = 0, ncols = 0;
    const int8_t *q8 = nullptr;
    const float *dx = nullptr, *xs = nullptr;
    bool valid = false;
} g_xi8_[GGML_HIP_MAX_BACKENDS];
#define g_xi8 (g_xi8_[g.slot])
void quantize_activation_i8(const ggml_tensor *src1, int qt, const int8_t **q8, const float **dx, const float **xs) {
    BK_ASSERT(src1->type == GGML_TYPE_F32 && src1->nb[0] == 4 && src1->ne[2] == 1 && src1->ne[3] == 1);
    const int64_t K = src1->ne[0], N = src1->ne[1], nb = K / 32;
    const bool f16_d = qt_f16d(qt);
    const float zp = qt == QT_Q4_0 ? 8.0f : qt == QT_Q5_0 ? 16.0f : 0.0f;
    // Q4_0 and Q5_0 differ only in the zero point, Q4_1 and Q5_1 not at all: the cache is keyed on what was produced
    const int key = f16_d ? (int)zp : 1000;
    if (!(g_xi8.valid && g_xi8.src_data == src1->data && g_xi8.qt == key && g_xi8.nb == nb && g_xi8.ncols == N)) {
        int8_t *o8 = (int8_t *)ws_alloc((size_t)N * K);
        float *od = (float *)ws_alloc((size_t)N * nb * 4);
        float *os = (float *)ws_alloc((size_t)N * nb * 4);
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)(K * N * 5));
        launch_quant_act_i8(f16_d, dev_ptr(src1), (int64_t)src1->nb[1], nb, N, zp, o8, od, os);
        HIP_CHECK(hipGetLastError());
        g_xi8.valid = true;
        g_xi8.src_data = src1->data;
        g_xi8.src_bytes = ggml_nbytes(src1);
        g_xi8.qt = key;
        g_xi8.nb = nb;
        g_xi8.ncols = N;
        g_xi8.q8 = o8;
        g_xi8.dx = od;
        g_xi8.xs = os;
    }
    *q8 = g_xi8.q8;
    *dx = g_xi8.dx;
    *xs = g_xi8.xs;
}
template <int QT>
void launch_mmq_i8(const MmqI8Args &a, dim3 grid) {
    lds_opt_in<k_mmq_i8<QT>>(I8_LDS, I8_LDS);
    g.stat_mmq[Backend::MMQ_K_I8]++;
    hipLaunchKernelGGL(k_mmq_i8<QT>, grid, dim3(256), I8_LDS, g.stream, a);
}

// ---- K-quant mat-vec (kernels/kquant.h): Q8_K activations (ggml's vec_dot_type of every K-quant), one launch per
// chunk of up to 8 columns.  Prompt batches take the same kernel (weights streamed once per 8 tokens): there is no
// K-quant GEMM yet (DESIGN.md section 8).
struct XKBuf {
    const void *src_data = nullptr;
    size_t src_bytes = 0;
    int64_t nsb = 0, ncols = 0;
    KAct act{};
    bool valid = false;
} g_xk_[GGML_HIP_MAX_BACKENDS];
#define g_xk (g_xk_[g.slot])
KAct quantize_activation_k(const ggml_tensor *src1) {
    BK_ASSERT(src1->type == GGML_TYPE_F32 && src1->nb[0] == 4 && src1->ne[2] == 1 && src1->ne[3] == 1);
    const int64_t K = src1->ne[0], N = src1->ne[1], nsb = K / 256;
    if (!(g_xk.valid && g_xk.src_data == src1->data && g_xk.nsb == nsb && g_xk.ncols == N)) {
        int8_t *q8 = (int8_t *)ws_alloc((size_t)N * K);
        float *d8 = (float *)ws_alloc((size_t)N * nsb * 4);
        int16_t *bs = (int16_t *)ws_alloc((size_t)N * nsb * 32);
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)(K * N * 5));
        launch_quant_q8k(dev_ptr(src1), (int64_t)src1->nb[1], nsb, N, q8, d8, bs);
        HIP_CHECK(hipGetLastError());
        g_xk.valid = true;
        g_xk.src_data = src1->data;
        g_xk.src_bytes = ggml_nbytes(src1);
        g_xk.nsb = nsb;
        g_xk.ncols = N;
        g_xk.act = KAct{q8, d8, bs};
    }
    return g_xk.act;
}
template <int KT, int NCOLS>
void launch_mmvq_k(const MmvqKArgs &a, int nwg, size_t lds) {
    if constexpr (KT == KT_Q4_K || KT == KT_Q6_K) {
        lds_opt_in<k_mmvq_k<KT, NCOLS>>(lds, 150 * 1024);
        hipLaunchKernelGGL((k_mmvq_k<KT, NCOLS>), dim3(nwg), dim3(256), lds, g.stream, a);
    } else {
        lds_opt_in<k_mmvq_k2<KT, NCOLS>>(lds, 150 * 1024);
        hipLaunchKernelGGL((k_mmvq_k2<KT, NCOLS>), dim3(nwg), dim3(256), lds, g.stream, a);
    }
}
template <int KT>
void launch_mmvq_k_c(const MmvqKArgs &a, int ncols, int nwg, size_t lds) {
    switch (ncols) {
        case 1: launch_mmvq_k<KT, 1>(a, nwg, lds); break;
        case 2: launch_mmvq_k<KT, 2>(a, nwg, lds); break;
        case 4: launch_mmvq_k<KT, 4>(a, nwg, lds); break;
        default: launch_mmvq_k<KT, 8>(a, nwg, lds); break;
    }
}
bool mul_mat_k_gemm(const ggml_tensor *src0, const ggml_tensor *src1, ggml_tensor *dst);
void mul_mat_k(const ggml_tensor *src0, const ggml_tensor *src1, ggml_tensor *dst) {
    const int kt = kt_of(src0->type);
    const int64_t K = src1->ne[0], N = src1->ne[1], nsb = K / 256;
    BK_ASSERT(K % 256 == 0 && src0->ne[0] == K && dst->type == GGML_TYPE_F32 && dst->nb[0] == 4);
    if (g.opt_mmq_min > 0 && N >= g.opt_mmq_min && mul_mat_k_gemm(src0, src1, dst)) return;  // prompt batch: f16 GEMM
    const KWeight w = kweight_of(src0);
    const KAct act = quantize_activation_k(src1);
    const size_t col_lds = (size_t)K + (size_t)nsb * (4 + 64);
    if (col_lds > 150 * 1024) die("mul_mat: K=%lld too large for the LDS-staged K-quant mat-vec", (long long)K);
    const double sb_bytes = k_block_bytes(kt);
    int64_t c0 = 0;
    while (c0 < N) {
        int ncols = 8;
        while (ncols > 1 && (ncols > N - c0 || (size_t)ncols * col_lds > 150 * 1024)) ncols >>= 1;
        MmvqKArgs a;
        a.w = w;
        a.x.q8 = act.q8 + c0 * K;
        a.x.d8 = act.d8 + c0 * nsb;
        a.x.bs = act.bs + c0 * nsb * 16;
        a.dst = (float *)(dev_ptr(dst) + c0 * dst->nb[1]);
        a.ldd = (int64_t)dst->nb[1] / 4;
        a.res = nullptr;
        a.nseg = 1;
        const size_t lds = (size_t)ncols * col_lds;
        // enough workgroups to fill the CUs' wave slots at this LDS footprint, never more than one row per wave
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, (150 * 1024) / std::max<size_t>(lds, 1)));
        const int nwg = (int)std::min<int64_t>((w.M + 3) / 4, (int64_t)g.num_cus * per_cu);
        Timed tm(GGML_HIP_KCLASS_MMVQ, (double)w.M * nsb * sb_bytes + (double)w.M * ncols * 4 + (double)lds);
        with_kt(kt, [&](auto KT) { launch_mmvq_k_c<CT(KT)>(a, ncols, nwg, lds); });
        HIP_CHECK(hipGetLastError());
        c0 += ncols;
    }
}
// rows of a planar K weight dequantized to f32 (the decoders of get_rows): dst[r * ldd + k]
void dequant_k_rows(const KWeight &w, const int *ids, int64_t rows, float *dst, int64_t ldd) {
    const dim3 grid((unsigned)((w.nsb * (w.kt == KT_Q4_K || w.kt == KT_Q6_K ? 8 : 16) + 255) / 256), (unsigned)rows);
    switch (w.kt) {
        case KT_Q4_K:
        case KT_Q6_K: hipLaunchKernelGGL(k_get_rows_k, grid, dim3(256), 0, g.stream, w, ids, dst, ldd); break;
        case KT_Q2_K: hipLaunchKernelGGL(k_get_rows_k2<KT_Q2_K>, grid, dim3(256), 0, g.stream, w, ids, dst, ldd); break;
        case KT_Q3_K: hipLaunchKernelGGL(k_get_rows_k2<KT_Q3_K>, grid, dim3(256), 0, g.stream, w, ids, dst, ldd); break;
        default: hipLaunchKernelGGL(k_get_rows_k2<KT_Q5_K>, grid, dim3(256), 0, g.stream, w, ids, dst, ldd); break;
    }
    HIP_CHECK(hipGetLastError());
}

// Resident f16 copy of a quantized weight (kernels/mmq_w16.h): created on first use by a prompt batch and kept as a CACHE:
// released with the weight's record, when option mmq_w16 is switched off, and whenever another allocation of the library
// fails (dev_malloc).  Returns false (and the GEMM dequantizes in LDS as before) when the option is off, K / 32 is odd,
// or HBM would be left with less than the headroom (option w16_headroom_gb, default 16 GB) after the allocation.
size_t w16_headroom() { return (size_t)std::max(0, g.opt_w16_headroom_gb) << 30; }
std::mutex g_w16_mu;  // creation of a copy (the record may be shared by the slots of one device)
size_t release_w16_copies() {
    // with several slots on this device a sibling's prompt plan may hold (or be running on) these very copies — also a sibling
    // that holds no session state at this moment (the model on this slot, its session on another: the plan there caches the
    // pointers and checks them against ITS slot's generation): they stay
    if (device_sharers() > 1 || device_siblings() > 0) return 0;
    size_t freed = 0;
    bool synced = false;
    for (auto *m : {&g.tensors, &g.auto_tensors})
        for (auto &kv : *m) {
            DevTensor *e = kv.second;
            if (!e->w16) continue;
            if (!synced && g.stream) {
                HIP_CHECK(hipStreamSynchronize(g.stream));
                synced = true;
            }
            HIP_CHECK(hipFree(e->w16));
            freed += e->w16_size;
            g.w16_bytes -= e->w16_size;
            e->w16 = nullptr;
            e->w16_size = 0;
            e->qw.w16 = nullptr;
        }
    if (freed) g.w16_gen++;  // prompt plans re-read their weights' w16 pointers at the next launch (plan_prompt.inc)
    return freed;
}
bool ensure_w16(DevTensor *e) {
    if (!e || !e->soa || !g.opt_mmq_w16 || e->qw.nb % 2 != 0) return false;
    std::lock_guard<std::mutex> w16_lk(g_w16_mu);
    if (e->w16) return true;
    const size_t bytes = (size_t)e->qw.M * e->qw.nb * 64;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + w16_headroom()) return false;
    char *w16 = nullptr;
    if (hipMalloc((void **)&w16, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    g_backends[e->slot].w16_bytes += bytes;  // accounted where the record lives (and is freed)
    e->w16_size = bytes;
    const bool shared = device_sharers() > 1;
    if (!shared) e->w16 = w16;
    const unsigned nblk = (unsigned)((e->qw.M * e->qw.nb + 255) / 256);
    with_qt(e->qw.qt, [&](auto QT) { hipLaunchKernelGGL(k_dequant_w16<CT(QT)>, dim3(nblk), dim3(256), 0, g.stream, e->qw, (_Float16 *)w16); },
            "w16: bad weight type");
    HIP_CHECK(hipGetLastError());
    if (shared) {  // another slot's stream may read the copy as soon as the pointer is visible: complete it first
        HIP_CHECK(hipStreamSynchronize(g.stream));
        e->w16 = w16;
    }
    e->qw.w16 = e->w16;
    return true;
}

// The same for a planar K-quant weight (kernels/kquant2.h): its rows dequantized by the get_rows decoders (f32, 8192 rows
// at a time through a temporary), rounded to f16 in the GEMM's k order.
bool ensure_w16_k(DevTensor *e) {
    if (!e || !e->ksoa || !g.opt_mmq_w16) return false;
    std::lock_guard<std::mutex> w16_lk(g_w16_mu);
    if (e->w16) return true;
    const int64_t M = e->kw.M, K = e->kw.nsb * 256, chunk = std::min<int64_t>(M, 8192);
    const size_t bytes = (size_t)M * K * 2, tmp_bytes = (size_t)chunk * K * 4;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < bytes + tmp_bytes + w16_headroom()) return false;
    float *tmp = nullptr;
    char *w16 = nullptr;
    if (hipMalloc((void **)&w16, bytes) != hipSuccess || hipMalloc((void **)&tmp, tmp_bytes) != hipSuccess) {
        (void)hipGetLastError();
        if (w16) HIP_CHECK(hipFree(w16));
        return false;
    }
    for (int64_t r0 = 0; r0 < M; r0 += chunk) {
        const int64_t n = std::min(chunk, M - r0);
        dequant_k_rows(kw_rows(e->kw, r0, n), nullptr, n, tmp, K);
        launch_f32_to_w16(tmp, n * K, (_Float16 *)w16 + r0 * K);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(g.stream));
    HIP_CHECK(hipFree(tmp));
    g_backends[e->slot].w16_bytes += bytes;
    e->w16_size = bytes;
    e->w16 = w16;  // published when complete (a sibling slot of this device may read it as soon as it sees the pointer)
    return true;
}

// The default prompt GEMM launch (f16 matrix cores): x16 = the activations after the Q8 pre-pass; dst[n * ldd + m].  Shared by the generic executor and the fused prompt plan.
// nseg > 1: up to three matrices with the same K in one launch (MmqArgs: nseg); `splits` 0 = chosen here.
struct MmqSegHost {
    QWeight w;
    float *dst;
    int64_t ldd;
};
int mmq_auto_splits(int tiles, int64_t nb, bool dst_contig) {
    // too few tiles to fill the chip (E x E at 512 tokens: 128 tiles for 256 CUs): split K in two, combined with
    // commutative (2-addend) f32 atomic adds into a zeroed dst
    const int nstage = (int)((nb + 1) / 2);
    return (tiles * 4 <= g.num_cus * 3 && nstage >= 16 && dst_contig) ? 2 : 1;
}
// Whether a prompt GEMM launch runs on the 256 x 256 kernel (kernels/mmq_w16_256.h): it needs every weight's resident f16
// copy, at least 160 tokens (62 % of a token tile) and enough (tile x split) items to keep >= 60 % of the CUs busy in every
// round.  The K split itself is NOT chosen here: it follows the 128-tile rule (mmq_auto_splits, per matrix) whatever the
// kernel, so that a fused launch of the prompt plan and the per-matrix launches of the node-by-node executor add the same
// partial sums (the kernels are bit-identical for equal splits).
bool mmq_use_t256(int nseg, const MmqSegHost *segs, int64_t N, int64_t nb, int splits) {
    if (!g.opt_mmq_t256 || !g.opt_mmq_w16 || nb % 2 != 0) return false;
    int tiles = 0;
    for (int i = 0; i < nseg; i++) {
        if (!segs[i].w.w16) return false;
        tiles += (int)((segs[i].w.M + T256_TM - 1) / T256_TM);
    }
    if (g.opt_mmq_t256 == 2) return true;  // tests: every launch that can run on it does
    if (N < 160) return false;
    tiles *= (int)((N + T256_TN - 1) / T256_TN);
    const int items = tiles * splits, rounds = (items + g.num_cus - 1) / g.num_cus;
    return items * 5 >= rounds * g.num_cus * 3;
}
void mmq_w16_256_launch(int nseg, const MmqSegHost *segs, const _Float16 *x16, int64_t N, int64_t nb, int splits, bool zero_dst,
                        int64_t split_stride) {
    MmqArgs a;
    memset(&a, 0, sizeof(a));
    a.w = segs[0].w;
    a.x = x16;
    a.dst = segs[0].dst;
    a.ldd = segs[0].ldd;
    a.M = a.w.M;
    a.N = N;
    a.nb = nb;
    a.nseg = nseg;
    int tiles_m = 0;
    double rows = 0;
    for (int i = 0; i < nseg; i++) {
        tiles_m += (int)((segs[i].w.M + T256_TM - 1) / T256_TM);
        rows += (double)segs[i].w.M;
        if (i < 2) a.tile_end[i] = tiles_m;
    }
    if (nseg > 1) { a.wb = segs[1].w; a.dst_b = segs[1].dst; a.ldd_b = segs[1].ldd; }
    if (nseg > 2) { a.wc = segs[2].w; a.dst_c = segs[2].dst; a.ldd_c = segs[2].ldd; }
    a.tiles_n = (int)((N + T256_TN - 1) / T256_TN);
    a.split_stride = splits > 1 ? split_stride : 0;
    if (splits > 1 && zero_dst && !split_stride)
        for (int i = 0; i < nseg; i++) HIP_CHECK(hipMemsetAsync(segs[i].dst, 0, (size_t)segs[i].w.M * N * 4, g.stream));
    lds_opt_in<k_mmq_w16_256<0>>(T256_LDS, T256_LDS);
    const int tiles_total = tiles_m * a.tiles_n, n_items = tiles_total * splits;
    Timed tm(GGML_HIP_KCLASS_MMQ_MFMA, 2.0 * rows * (double)N * (double)(nb * 32));
    g.stat_mmq[Backend::MMQ_K_W16_256]++;
    const dim3 grid((unsigned)std::min(n_items, g.num_cus));
    hipLaunchKernelGGL(k_mmq_w16_256<0>, grid, dim3(512), T256_LDS, g.stream, a, n_items, tiles_total, splits);
    HIP_CHECK(hipGetLastError());
}
void mmq_f16_launch_multi(int qt, int nseg, const MmqSegHost *segs, const _Float16 *x16, int64_t N, int64_t nb, bool dst_contig,
                          int splits, bool zero_dst, int64_t split_stride = 0) {
    BK_ASSERT(x16);
    if (splits <= 0) {
        int t128 = 0;
        for (int i = 0; i < nseg; i++) t128 += (int)((segs[i].w.M + MMQ_TM - 1) / MMQ_TM);
        splits = mmq_auto_splits(t128 * (int)((N + MMQ_TN - 1) / MMQ_TN), nb, dst_contig);
    }
    if (mmq_use_t256(nseg, segs, N, nb, splits)) {
        mmq_w16_256_launch(nseg, segs, x16, N, nb, splits, zero_dst, split_stride);
        return;
    }
    MmqArgs a;
    memset(&a, 0, sizeof(a));
    a.w = segs[0].w;
    a.x = x16;
    a.dst = segs[0].dst;
    a.ldd = segs[0].ldd;
    a.M = a.w.M;
    a.N = N;
    a.nb = nb;
    a.nseg = nseg;
    int tiles_m = 0;
    double rows = 0;
    bool all_w16 = g.opt_mmq_w16 != 0;
    for (int i = 0; i < nseg; i++) {
        tiles_m += (int)((segs[i].w.M + MMQ_TM - 1) / MMQ_TM);
        rows += (double)segs[i].w.M;
        if (i < 2) a.tile_end[i] = tiles_m;
        all_w16 = all_w16 && segs[i].w.w16 != nullptr;
    }
    if (nseg > 1) { a.wb = segs[1].w; a.dst_b = segs[1].dst; a.ldd_b = segs[1].ldd; }
    if (nseg > 2) { a.wc = segs[2].w; a.dst_c = segs[2].dst; a.ldd_c = segs[2].ldd; }
    a.tiles_n = (int)((N + MMQ_TN - 1) / MMQ_TN);
    a.split_stride = splits > 1 ? split_stride : 0;
    if (splits > 1 && zero_dst && !split_stride)
        for (int i = 0; i < nseg; i++) HIP_CHECK(hipMemsetAsync(segs[i].dst, 0, (size_t)segs[i].w.M * N * 4, g.stream));
    if (nb % 2 != 0) {  // K/32 odd (no LLaMA size; the 352-wide test models): one workgroup per tile, register-staged (kernels/mmq_plain.h)
        const dim3 grid((unsigned)(tiles_m * a.tiles_n), (unsigned)splits);
        Timed tm(GGML_HIP_KCLASS_MMQ_MFMA, 2.0 * rows * (double)N * (double)(nb * 32));
        g.stat_mmq[Backend::MMQ_K_PLAIN]++;
        with_qt(qt, [&](auto QT) {
            lds_opt_in<k_mmq<CT(QT)>>(MMQ_LDS, MMQ_LDS);  // 73.7 KB of dynamic LDS
            hipLaunchKernelGGL(k_mmq<CT(QT)>, grid, dim3(256), MMQ_LDS, g.stream, a);
        }, "mmq: bad weight type");
        HIP_CHECK(hipGetLastError());
        return;
    }
    // persistent 128 x 128 x 64 GEMM: one 8-wave workgroup per CU walks the (tile x K split) items
    const int tiles_total = tiles_m * a.tiles_n, n_items = tiles_total * splits;
    const dim3 pgrid((unsigned)std::min(n_items, g.num_cus));
    Timed tm(GGML_HIP_KCLASS_MMQ_MFMA, 2.0 * rows * (double)N * (double)(nb * 32));
    if (all_w16) {  // both operands by DMA from resident f16 copies (kernels/mmq_w16.h)
        lds_opt_in<k_mmq_w16_p8>(W16_LDS, W16_LDS);
        g.stat_mmq[Backend::MMQ_K_W16_P8]++;
        hipLaunchKernelGGL(k_mmq_w16_p8, pgrid, dim3(512), W16_LDS, g.stream, a, n_items, tiles_total, splits);
        HIP_CHECK(hipGetLastError());
        return;
    }
    // no resident copy (HBM full, option off): quantized blocks by LDS-DMA, dequantized in LDS (kernels/mmq_dmap8.h)
    g.stat_mmq[Backend::MMQ_K_DMA_P8]++;
    with_qt(qt, [&](auto QT) {
        lds_opt_in<k_mmq_dma_p8<CT(QT)>>(Dma8<CT(QT)>::LDS, Dma8<CT(QT)>::LDS);
        hipLaunchKernelGGL(k_mmq_dma_p8<CT(QT)>, pgrid, dim3(512), Dma8<CT(QT)>::LDS, g.stream, a, n_items, tiles_total, splits);
    }, "mmq: bad weight type");
    HIP_CHECK(hipGetLastError());
}

void mmq_f16_launch(int qt, const QWeight &w, const _Float16 *x16, float *dst, int64_t ldd, int64_t N, int64_t nb, bool dst_contig) {
    const MmqSegHost seg{w, dst, ldd};
    mmq_f16_launch_multi(qt, 1, &seg, x16, N, nb, dst_contig, 0, true);
}

// Quantized GEMM on the f16 matrix cores (kernels/mmq.h); the `algo_bytes` slot of the MMQ_MFMA timing class
// carries FLOPs (2*M*N*K), the unit that class is bounded by.
void mul_mat_q_mfma(const ggml_tensor *src0, const ggml_tensor *src1, ggml_tensor *dst) {
    const int qt = qt_of(src0->type);
    const int64_t K = src1->ne[0], N = src1->ne[1], nb = K / 32;
    const bool f16_d = qt_f16d(qt);
    if (g.opt_mmq_i8 && nb % 2 == 0) {  // integer matrix cores: ggml's exact block dots (kernels/mmq_i8.h)
        MmqI8Args ia;
        ia.w = qweight_of(src0);
        quantize_activation_i8(src1, qt, &ia.x8, &ia.dx, &ia.xs);
        ia.dst = (float *)dev_ptr(dst);
        ia.ldd = (int64_t)dst->nb[1] / 4;
        ia.M = ia.w.M;
        ia.N = N;
        ia.nb = nb;
        const int tiles_m = (int)((ia.M + MMQ_TM - 1) / MMQ_TM);
        ia.tiles_n = (int)((N + MMQ_TN - 1) / MMQ_TN);
        const int nstage = (int)(nb / 2);
        const int splits = (tiles_m * ia.tiles_n * 2 <= g.num_cus * 3 && nstage >= 16 && dst->nb[0] == 4 &&
                            ggml_is_contiguous(dst)) ? 2 : 1;  // two workgroups per CU: fewer than 1.5 tiles per slot -> split K
        if (splits > 1) HIP_CHECK(hipMemsetAsync(ia.dst, 0, (size_t)ia.M * N * 4, g.stream));
        const dim3 grid((unsigned)(tiles_m * ia.tiles_n), (unsigned)splits);
        Timed tm(GGML_HIP_KCLASS_MMQ_MFMA, 2.0 * (double)ia.M * (double)N * (double)K);
        with_qt(qt, [&](auto QT) { launch_mmq_i8<CT(QT)>(ia, grid); }, "mmq: bad weight type");
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (N >= W16_MIN_TOKENS) {  // a resident weight meeting a real prompt batch gets its f16 copy here too (the prompt plan
        DevTensor *e = extra_of(src0);  // makes them for a whole model at once, plan_build.inc)
        if (!e) e = find_tensor((uintptr_t)src0->data);
        if (e && e->soa && (uintptr_t)src0->data == e->host) ensure_w16(e);
    }
    const _Float16 *x16 = quantize_activation_f16(src1, f16_d);
    mmq_f16_launch(qt, qweight_of(src0), x16, (float *)dev_ptr(dst), (int64_t)dst->nb[1] / 4, N, nb,
                   dst->nb[0] == 4 && ggml_is_contiguous(dst));
}

// K-quant prompt batch on the f16 GEMM: the weight's resident f16 copy x the activations after their Q8_K round trip
// (f16(d8 * q): what ggml's K-quant dots see of src1).  Same kernels and tile rules as the other formats; the f16 rounding
// of both operands is the approximation those already make.  false = not applicable here (the caller streams the weight
// through the mat-vec kernel instead): options off, a view / workspace weight, fewer than 64 tokens without a copy yet, no HBM.
bool mul_mat_k_gemm(const ggml_tensor *src0, const ggml_tensor *src1, ggml_tensor *dst) {
    if (!g.opt_mmq_w16 || g.opt_mmq_i8) return false;
    if (dst->type != GGML_TYPE_F32 || dst->nb[0] != 4 || src1->ne[2] != 1 || src1->ne[3] != 1) return false;
    DevTensor *e = extra_of(src0);
    if (!e) e = find_tensor((uintptr_t)src0->data);
    if (!(e && e->ksoa && (uintptr_t)src0->data == e->host)) return false;
    const int64_t K = src1->ne[0], N = src1->ne[1], nsb = K / 256;
    if (!e->w16 && N < W16_MIN_TOKENS) return false;
    if (!ensure_w16_k(e)) return false;
    _Float16 *x16 = (_Float16 *)ws_alloc((size_t)N * K * 2);
    {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)(K * N * 6));
        launch_quant_act_f16_k(dev_ptr(src1), (int64_t)src1->nb[1], nsb, N, x16);
        HIP_CHECK(hipGetLastError());
    }
    QWeight w;
    memset(&w, 0, sizeof(w));
    w.M = e->kw.M;
    w.nb = K / 32;
    w.qt = QT_Q8_0;  // never read: every kernel that takes a resident copy reads only w16
    w.w16 = e->w16;
    mmq_f16_launch(QT_Q8_0, w, x16, (float *)dev_ptr(dst), (int64_t)dst->nb[1] / 4, N, K / 32,
                   ggml_is_contiguous(dst));
    return true;
}

int pick_rows(int64_t M) {
    return M >= 16384 ? 2 : 1;
}

// Quantized mat-vec over up to 3 weight matrices sharing src1 (same type, same K).
void mul_mat_q(int nmat, const ggml_tensor *const *src0s, const ggml_tensor *src1, ggml_tensor *const *dsts) {
    const int qt = qt_of(src0s[0]->type);
    const int64_t K = src1->ne[0], N = src1->ne[1], nb = K / 32;
    BK_ASSERT(K % 32 == 0);
    QWeight ws[3];
    for (int i = 0; i < nmat; i++) {
        BK_ASSERT(src0s[i]->type == src0s[0]->type && src0s[i]->ne[0] == K);
        BK_ASSERT(dsts[i]->type == GGML_TYPE_F32 && dsts[i]->nb[0] == 4);
        ws[i] = qweight_of(src0s[i]);
    }
    if (g.opt_mmq_min > 0 && N >= g.opt_mmq_min) {  // prompt batch: MFMA GEMM
        for (int i = 0; i < nmat; i++) mul_mat_q_mfma(src0s[i], src1, dsts[i]);
        return;
    }
    const bool f16_d = qt_f16d(qt);
    const QAct act = quantize_activation(src1, f16_d);
    const int64_t max_cols_lds = (int64_t)(64 * 1024) / (nb * 40);
    if (max_cols_lds < 1) die("mul_mat: K=%lld too large for the LDS-staged mat-vec", (long long)K);
    int64_t c0 = 0;
    while (c0 < N) {
        int ncols = 8;
        while (ncols > 1 && (ncols > N - c0 || ncols > max_cols_lds)) ncols >>= 1;
        MmvqArgs a;
        memset(&a, 0, sizeof(a));
        a.nseg = nmat;
        a.nb = nb;
        a.x.lo = act.lo + c0 * nb;
        a.x.hi = act.hi + c0 * nb;
        a.x.d = act.d + c0 * nb;
        a.x.sum = act.sum + c0 * nb;
        int nwg = 0;
        int64_t Mmax = 0;
        for (int i = 0; i < nmat; i++) Mmax = std::max(Mmax, ws[i].M);
        const int R = pick_rows(Mmax);
        double bytes = 0;
        for (int i = 0; i < nmat; i++) {
            a.seg[i].w = ws[i];
            a.seg[i].dst = (float *)(dev_ptr(dsts[i]) + c0 * dsts[i]->nb[1]);
            a.seg[i].ldd = (int64_t)dsts[i]->nb[1] / 4;
            a.seg[i].wg_begin = nwg;
            nwg += (int)((ws[i].M + 4 * R - 1) / (4 * R));
            bytes += (double)ws[i].M * nb * blk_bytes(qt) + (double)ws[i].M * ncols * 4;
        }
        bytes += (double)ncols * nb * 40;
        Timed tm(GGML_HIP_KCLASS_MMVQ, bytes);
        launch_mmvq(qt, a, ncols, R, nwg, (size_t)ncols * nb * 40);
        c0 += ncols;
    }
}

void op_mul_mat(ggml_tensor *dst) {
    const ggml_tensor *a = dst->src[0], *b = dst->src[1];
    if (qt_of(a->type) >= 0) {
        const ggml_tensor *s0[1] = {a};
        ggml_tensor *d[1] = {dst};
        mul_mat_q(1, s0, b, d);
        return;
    }
    if (kt_of(a->type) >= 0) {
        mul_mat_k(a, b, dst);
        return;
    }
    BK_ASSERT(b->type == GGML_TYPE_F32 && dst->type == GGML_TYPE_F32);
    BK_ASSERT(b->nb[0] == 4);
    const TView va = view_of(a), vb = view_of(b), vd = view_of(dst);
    const dim3 grid((unsigned)((a->ne[1] + 3) / 4), (unsigned)b->ne[1], (unsigned)(b->ne[2] * b->ne[3]));
    const double bytes = (double)ggml_nelements(a) * ggml_element_size(a) * 1.0 + (double)ggml_nelements(b) * 4 +
                         (double)ggml_nelements(dst) * 4;
    Timed tm(GGML_HIP_KCLASS_ATTN, bytes);
    if (a->type == GGML_TYPE_F16) {
        BK_ASSERT(a->nb[0] == 2);
        const bool aligned = ((uintptr_t)va.p % 16 == 0) && a->nb[1] % 16 == 0 && a->nb[2] % 16 == 0 && a->nb[3] % 16 == 0;
        if (g.opt_mmq_min > 0 && b->ne[1] >= g.opt_mmq_min && aligned && dst->nb[0] == 4) {
            // prompt batch: both attention products on the f16 matrix cores (kernels/gemm_f16.h)
            GemmF16Args ga;
            ga.a = va.p; ga.a_nb1 = a->nb[1]; ga.a_nb2 = a->nb[2]; ga.a_nb3 = a->nb[3];
            ga.b = vb.p; ga.b_nb1 = b->nb[1]; ga.b_nb2 = b->nb[2]; ga.b_nb3 = b->nb[3];
            ga.d = vd.p; ga.d_nb1 = dst->nb[1]; ga.d_nb2 = dst->nb[2]; ga.d_nb3 = dst->nb[3];
            ga.M = a->ne[1]; ga.N = b->ne[1]; ga.K = a->ne[0];
            ga.ne12 = b->ne[2]; ga.r2 = b->ne[2] / a->ne[2]; ga.r3 = b->ne[3] / a->ne[3];
            ga.tiles_n = (int)((ga.N + 127) / 128);
            ga.causal = 0;
            ga.causal_past = 0;
            const int tiles_m = (int)((ga.M + 127) / 128);
            lds_opt_in<k_gemm_f16>(MMQ_LDS, MMQ_LDS);
            hipLaunchKernelGGL(k_gemm_f16, dim3((unsigned)(tiles_m * ga.tiles_n), (unsigned)(b->ne[2] * b->ne[3])), dim3(256),
                               MMQ_LDS, g.stream, ga);
        } else
            hipLaunchKernelGGL(k_mul_mat_f16, grid, dim3(256), 0, g.stream, va, vb, vd);
    } else if (a->type == GGML_TYPE_F32) {
        BK_ASSERT(a->nb[0] == 4);
        hipLaunchKernelGGL(k_mul_mat_f32, grid, dim3(256), 0, g.stream, va, vb, vd);
    } else {
        die("mul_mat: unsupported src0 type %s", ggml_type_name(a->type));
    }
    HIP_CHECK(hipGetLastError());
}

void op_rms_norm(ggml_tensor *dst, const ggml_tensor *weight /* nullable: fused mul */, ggml_tensor *out) {
    const ggml_tensor *x = dst->src[0];
    BK_ASSERT(x->type == GGML_TYPE_F32 && x->nb[0] == 4 && out->nb[0] == 4);
    float eps;
    memcpy(&eps, dst->op_params, sizeof(float));
    const int64_t rows = ggml_nrows(x);
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)ggml_nelements(x) * 8);
    if (weight) {
        BK_ASSERT(is_contig_f32(weight) && weight->ne[0] == x->ne[0] && ggml_nelements(weight) == x->ne[0]);
        hipLaunchKernelGGL(k_rms_norm<true>, dim3((unsigned)rows), dim3(256), 0, g.stream, view_of(x), view_of(out),
                           (const float *)dev_ptr(weight), eps);
    } else {
        hipLaunchKernelGGL(k_rms_norm<false>, dim3((unsigned)rows), dim3(256), 0, g.stream, view_of(x), view_of(out),
                           (const float *)nullptr, eps);
    }
    HIP_CHECK(hipGetLastError());
}

void op_norm(ggml_tensor *dst) {
    const ggml_tensor *x = dst->src[0];
    BK_ASSERT(x->type == GGML_TYPE_F32 && x->nb[0] == 4 && dst->nb[0] == 4);
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)ggml_nelements(x) * 8);
    hipLaunchKernelGGL(k_norm, dim3((unsigned)ggml_nrows(x)), dim3(256), 0, g.stream, view_of(x), view_of(dst), 1e-5f);
    HIP_CHECK(hipGetLastError());
}

void op_bin(ggml_tensor *dst, int op) {
    const ggml_tensor *a = dst->src[0], *b = dst->src[1];
    BK_ASSERT(dst->type == GGML_TYPE_F32);
    const int64_t n = ggml_nelements(dst);
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)n * 12);
    if (op == BIN_REPEAT) {
        BK_ASSERT(a->type == GGML_TYPE_F32);
        const TView va = view_of(a), vd = view_of(dst);
        hipLaunchKernelGGL(k_bin<BIN_REPEAT>, grid1(n), dim3(256), 0, g.stream, va, va, vd, n);
    } else {
        BK_ASSERT(a->type == GGML_TYPE_F32 && b->type == GGML_TYPE_F32);
        const TView va = view_of(a), vb = view_of(b), vd = view_of(dst);
        const bool same = is_contig_f32(a) && is_contig_f32(b) && is_contig_f32(dst) && ggml_nelements(a) == n &&
                          ggml_nelements(b) == n && n % 4 == 0 &&
                          (((uintptr_t)va.p | (uintptr_t)vb.p | (uintptr_t)vd.p) & 15) == 0;
        if (same) {
            if (op == BIN_ADD)
                hipLaunchKernelGGL(k_bin4<BIN_ADD>, grid1(n / 4), dim3(256), 0, g.stream, (const f32x4 *)va.p,
                                   (const f32x4 *)vb.p, (f32x4 *)vd.p, n / 4);
            else
                hipLaunchKernelGGL(k_bin4<BIN_MUL>, grid1(n / 4), dim3(256), 0, g.stream, (const f32x4 *)va.p,
                                   (const f32x4 *)vb.p, (f32x4 *)vd.p, n / 4);
        } else if (op == BIN_ADD)
            hipLaunchKernelGGL(k_bin<BIN_ADD>, grid1(n), dim3(256), 0, g.stream, va, vb, vd, n);
        else
            hipLaunchKernelGGL(k_bin<BIN_MUL>, grid1(n), dim3(256), 0, g.stream, va, vb, vd, n);
    }
    HIP_CHECK(hipGetLastError());
}

// ggml_add(W, x) with W quantized (Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0, Q2_K .. Q6_K) or f16 and x f32: the add of a LoRA patch
// (lora.rs:126), ggml's add_q_f32 / add_f16_f32.  dst has W's type; same shape only, as upstream asserts.
void op_add_lowp(ggml_tensor *dst) {
    const ggml_tensor *a = dst->src[0], *b = dst->src[1];
    const int kt = kt_of(a->type);
    if (kt >= 0 && a->ne[0] % 256 != 0)
        die("add: '%s' is %s with ne0 = %lld: a K-quant src0 needs ne0 %% 256 == 0", a->name, ggml_type_name(a->type), (long long)a->ne[0]);
    const int qt = qt_of(a->type);
    if (qt < 0 && kt < 0 && a->type != GGML_TYPE_F16)
        die("add: '%s' is %s: no device add for this src0 type", a->name, ggml_type_name(a->type));
    bool same = true;
    for (int i = 0; i < 4; i++) same = same && a->ne[i] == b->ne[i] && a->ne[i] == dst->ne[i];
    if (!same)
        die("add: '%s' (%s, [%lld, %lld, %lld, %lld]) and '%s' ([%lld, %lld, %lld, %lld]) must have the same shape when src0 "
            "is not f32",
            a->name, ggml_type_name(a->type), (long long)a->ne[0], (long long)a->ne[1], (long long)a->ne[2],
            (long long)a->ne[3], b->name, (long long)b->ne[0], (long long)b->ne[1], (long long)b->ne[2], (long long)b->ne[3]);
    if (b->type != GGML_TYPE_F32 || dst->type != a->type)
        die("add: '%s' (%s) + '%s' (%s) -> %s: the second operand must be f32 and the result of the first operand's type",
            a->name, ggml_type_name(a->type), b->name, ggml_type_name(b->type), ggml_type_name(dst->type));
    const size_t es = ggml_type_size(a->type);
    BK_ASSERT(b->nb[0] == 4 && a->nb[0] == es && dst->nb[0] == es);
    const TView va = view_of(a), vb = view_of(b), vd = view_of(dst);
    BK_ASSERT((((uintptr_t)va.p | (uintptr_t)vd.p | a->nb[1] | a->nb[2] | a->nb[3] | dst->nb[1] | dst->nb[2] | dst->nb[3]) & 1) == 0);
    BK_ASSERT((((uintptr_t)vb.p | b->nb[1] | b->nb[2] | b->nb[3]) & 3) == 0);
    const int64_t n = ggml_nelements(a);
    if (n == 0) return;
    if (a->type == GGML_TYPE_F16) {
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)n * 8);
        hipLaunchKernelGGL(k_add_f16, grid1(n), dim3(256), 0, g.stream, va, vb, vd, n);
    } else if (kt >= 0) {  // one wave per super-block, four per workgroup (kernels/lora.h k_add_k)
        const int64_t spr = a->ne[0] / 256, nsb = n / 256;
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)nsb * (2.0 * (double)es + 1024.0));
        const dim3 grid((unsigned)((nsb + 3) / 4));
        switch (kt) {
            case KT_Q2_K: hipLaunchKernelGGL(k_add_k<KT_Q2_K>, grid, dim3(256), 0, g.stream, va, vb, vd, spr, nsb); break;
            case KT_Q3_K: hipLaunchKernelGGL(k_add_k<KT_Q3_K>, grid, dim3(256), 0, g.stream, va, vb, vd, spr, nsb); break;
            case KT_Q4_K: hipLaunchKernelGGL(k_add_k<KT_Q4_K>, grid, dim3(256), 0, g.stream, va, vb, vd, spr, nsb); break;
            case KT_Q5_K: hipLaunchKernelGGL(k_add_k<KT_Q5_K>, grid, dim3(256), 0, g.stream, va, vb, vd, spr, nsb); break;
            default: hipLaunchKernelGGL(k_add_k<KT_Q6_K>, grid, dim3(256), 0, g.stream, va, vb, vd, spr, nsb); break;
        }
    } else {
        BK_ASSERT(a->ne[0] % 32 == 0);
        const int64_t bpr = a->ne[0] / 32, nblocks = n / 32;
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)nblocks * (2.0 * (double)es + 128.0));
        switch (a->type) {
            case GGML_TYPE_Q4_0: hipLaunchKernelGGL(k_add_q<GGML_TYPE_Q4_0>, grid1(nblocks), dim3(256), 0, g.stream, va, vb, vd, bpr, nblocks); break;
            case GGML_TYPE_Q4_1: hipLaunchKernelGGL(k_add_q<GGML_TYPE_Q4_1>, grid1(nblocks), dim3(256), 0, g.stream, va, vb, vd, bpr, nblocks); break;
            case GGML_TYPE_Q5_0: hipLaunchKernelGGL(k_add_q<GGML_TYPE_Q5_0>, grid1(nblocks), dim3(256), 0, g.stream, va, vb, vd, bpr, nblocks); break;
            case GGML_TYPE_Q5_1: hipLaunchKernelGGL(k_add_q<GGML_TYPE_Q5_1>, grid1(nblocks), dim3(256), 0, g.stream, va, vb, vd, bpr, nblocks); break;
            default: hipLaunchKernelGGL(k_add_q<GGML_TYPE_Q8_0>, grid1(nblocks), dim3(256), 0, g.stream, va, vb, vd, bpr, nblocks); break;
        }
    }
    HIP_CHECK(hipGetLastError());
}

void op_unary(ggml_tensor *dst, const ggml_tensor *mul_b /* nullable: fused silu*b */, ggml_tensor *out) {
    const ggml_tensor *a = dst->src[0];
    const int32_t uop = dst->op_params[0];
    BK_ASSERT(is_contig_f32(a) && is_contig_f32(out));
    const int64_t n = ggml_nelements(a);
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)n * (mul_b ? 12 : 8));
    const float *pa = (const float *)dev_ptr(a);
    float *pd = (float *)dev_ptr(out);
    if (uop == GGML_UNARY_OP_SILU) {
        if (mul_b) {
            BK_ASSERT(is_contig_f32(mul_b) && ggml_nelements(mul_b) == n);
            const float *pb = (const float *)dev_ptr(mul_b);
            if (n % 4 == 0 && (((uintptr_t)pa | (uintptr_t)pb | (uintptr_t)pd) & 15) == 0)
                hipLaunchKernelGGL((k_unary4<UN_SILU, true>), grid1(n / 4), dim3(256), 0, g.stream, (const f32x4 *)pa,
                                   (const f32x4 *)pb, (f32x4 *)pd, n / 4);
            else
                hipLaunchKernelGGL((k_unary<UN_SILU, true>), grid1(n), dim3(256), 0, g.stream, pa, pb, pd, n);
        } else {
            hipLaunchKernelGGL((k_unary<UN_SILU, false>), grid1(n), dim3(256), 0, g.stream, pa, (const float *)nullptr,
                               pd, n);
        }
    } else if (uop == GGML_UNARY_OP_GELU) {
        BK_ASSERT(!mul_b);
        hipLaunchKernelGGL((k_unary<UN_GELU, false>), grid1(n), dim3(256), 0, g.stream, pa, (const float *)nullptr, pd,
                           n);
    } else {
        die("unary op %d is outside the accelerated path", (int)uop);
    }
    HIP_CHECK(hipGetLastError());
}

void op_scale(ggml_tensor *dst) {
    const ggml_tensor *a = dst->src[0], *s = dst->src[1];
    BK_ASSERT(is_contig_f32(a) && is_contig_f32(dst) && s->type == GGML_TYPE_F32);
    const int64_t n = ggml_nelements(a);
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)n * 8);
    hipLaunchKernelGGL(k_scale, grid1(n), dim3(256), 0, g.stream, (const float *)dev_ptr(a), (const float *)dev_ptr(s),
                       (float *)dev_ptr(dst), n);
    HIP_CHECK(hipGetLastError());
}

void op_diag_mask_inf(ggml_tensor *dst) {
    const ggml_tensor *a = dst->src[0];
    BK_ASSERT(is_contig_f32(a) && is_contig_f32(dst));
    const int64_t n = ggml_nelements(a);
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)n * 8);
    hipLaunchKernelGGL(k_diag_mask_inf, grid1(n), dim3(256), 0, g.stream, (const float *)dev_ptr(a),
                       (float *)dev_ptr(dst), a->ne[0], a->ne[1], n, (int)dst->op_params[0]);
    HIP_CHECK(hipGetLastError());
}

void op_soft_max(ggml_tensor *dst) {
    const ggml_tensor *a = dst->src[0];
    BK_ASSERT(is_contig_f32(a) && is_contig_f32(dst));
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)ggml_nelements(a) * 8);
    hipLaunchKernelGGL(k_soft_max<false>, dim3((unsigned)ggml_nrows(a)), dim3(256), 0, g.stream,
                       (const float *)dev_ptr(a), (float *)dev_ptr(dst), a->ne[0], a->ne[1], (const float *)nullptr, 0);
    HIP_CHECK(hipGetLastError());
}

// fused scale -> diag_mask_inf -> soft_max (all three in-place on the KQ tensor)
void op_scale_mask_softmax(const ggml_tensor *kq, const ggml_tensor *scale, int n_past, ggml_tensor *out) {
    BK_ASSERT(is_contig_f32(kq) && is_contig_f32(out));
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)ggml_nelements(kq) * 8);
    hipLaunchKernelGGL(k_soft_max<true>, dim3((unsigned)ggml_nrows(kq)), dim3(256), 0, g.stream,
                       (const float *)dev_ptr(kq), (float *)dev_ptr(out), kq->ne[0], kq->ne[1],
                       (const float *)dev_ptr(scale), n_past);
    HIP_CHECK(hipGetLastError());
}

// ggml_compute_forward_alibi_f32's slope table, with the C library's powf: heads k < n_floor = 2^floor(log2 n_head) take
// m0^(k+1), the rest m1^(2(k - n_floor) + 1)
AlibiSlopes alibi_slopes(const ggml_tensor *alibi) {
    const int n_head = alibi->op_params[1];
    float bias_max;
    memcpy(&bias_max, alibi->op_params + 2, sizeof(float));
    BK_ASSERT(n_head >= 1 && n_head <= 256);
    AlibiSlopes s = {};
    const int n_floor = 1 << (int)floor(log2(n_head));
    const float m0 = powf(2.0f, -(bias_max) / n_floor);
    const float m1 = powf(2.0f, -(bias_max / 2.0f) / n_floor);
    for (int k = 0; k < n_head; k++) s.m[k] = k < n_floor ? powf(m0, k + 1) : powf(m1, 2 * (k - n_floor) + 1);
    return s;
}

// KQ [n_past + N, N, n_head] f32 with contiguous rows (the layout ggml_alibi accepts); in place on its view
void op_alibi(ggml_tensor *dst) {
    const ggml_tensor *a = dst->src[0];
    BK_ASSERT(is_contig_f32(a) && dst->data == a->data && a->ne[2] == dst->op_params[1] && a->ne[3] == 1);
    const int64_t n = ggml_nelements(a);
    if (n == 0) return;
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)n * 8);
    hipLaunchKernelGGL(k_alibi, grid1(n), dim3(256), 0, g.stream, (float *)dev_ptr(dst), a->ne[0], a->ne[1], n,
                       alibi_slopes(dst));
    HIP_CHECK(hipGetLastError());
}

// fused scale -> alibi -> diag_mask_inf -> soft_max: reads KQ, writes P (which may alias KQ)
void op_scale_alibi_mask_softmax(const ggml_tensor *kq, const ggml_tensor *scale, const ggml_tensor *alibi, int n_past,
                                 ggml_tensor *out) {
    BK_ASSERT(is_contig_f32(kq) && is_contig_f32(out) && kq->ne[2] == alibi->op_params[1] && kq->ne[3] == 1);
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)ggml_nelements(kq) * 8);
    hipLaunchKernelGGL((k_soft_max<true, true>), dim3((unsigned)ggml_nrows(kq)), dim3(256), 0, g.stream,
                       (const float *)dev_ptr(kq), (float *)dev_ptr(out), kq->ne[0], kq->ne[1],
                       (const float *)dev_ptr(scale), n_past, alibi_slopes(alibi));
    HIP_CHECK(hipGetLastError());
}

void op_rope(ggml_tensor *dst) {
    const ggml_tensor *a = dst->src[0];
    BK_ASSERT(a->type == GGML_TYPE_F32 && dst->type == GGML_TYPE_F32);
    const int n_past = dst->op_params[0], n_dims = dst->op_params[1], mode = dst->op_params[2];
    float freq_base, freq_scale;
    memcpy(&freq_base, dst->op_params + 4, 4);
    memcpy(&freq_scale, dst->op_params + 5, 4);
    if (mode & 4) die("rope mode %d (GLM) is outside the accelerated path", mode);
    const float theta_scale = powf(freq_base, -2.0f / n_dims);
    if (mode & 2) {  // NeoX: GPT-NeoX, Falcon (kernels/ops.h k_rope_neox)
        BK_ASSERT(n_dims > 0 && n_dims % 2 == 0 && a->nb[0] == 4 && dst->nb[0] == 4);
        const TView va = view_of(a), vd = view_of(dst);
        const int in_place = va.p == vd.p;
        const int64_t per_row = in_place ? (a->ne[0] / n_dims) * (n_dims / 2) : a->ne[0];
        const int64_t total = per_row * a->ne[1] * a->ne[2] * a->ne[3];
        if (total == 0) return;
        Timed tm(GGML_HIP_KCLASS_OTHER, (double)ggml_nelements(a) * 8);
        hipLaunchKernelGGL(k_rope_neox, grid1(total), dim3(256), 0, g.stream, va, vd, n_past, n_dims, theta_scale,
                           freq_scale, mode, per_row, in_place);
        HIP_CHECK(hipGetLastError());
        return;
    }
    BK_ASSERT(a->ne[0] % 2 == 0);
    const int64_t total = (a->ne[0] / 2) * a->ne[1] * a->ne[2] * a->ne[3];
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)ggml_nelements(a) * 8);
    hipLaunchKernelGGL(k_rope, grid1(total), dim3(256), 0, g.stream, view_of(a), view_of(dst), n_past, theta_scale,
                       freq_scale, mode);
    HIP_CHECK(hipGetLastError());
}

void op_cpy(const ggml_tensor *src, ggml_tensor *dst) {
    const int64_t n = ggml_nelements(src);
    BK_ASSERT(n == ggml_nelements(dst));
    const TView vs = view_of(src), vd = view_of(dst);
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)n * (ggml_element_size(src) + ggml_element_size(dst)));
    const ggml_type ts = src->type, td = dst->type;
    if (ts == GGML_TYPE_F32 && td == GGML_TYPE_F32)
        hipLaunchKernelGGL((k_cpy<float, float>), grid1(n), dim3(256), 0, g.stream, vs, vd, n);
    else if (ts == GGML_TYPE_F32 && td == GGML_TYPE_F16)
        hipLaunchKernelGGL((k_cpy<float, __half>), grid1(n), dim3(256), 0, g.stream, vs, vd, n);
    else if (ts == GGML_TYPE_F16 && td == GGML_TYPE_F16)
        hipLaunchKernelGGL((k_cpy<__half, __half>), grid1(n), dim3(256), 0, g.stream, vs, vd, n);
    else if (ts == GGML_TYPE_F16 && td == GGML_TYPE_F32)
        hipLaunchKernelGGL((k_cpy<__half, float>), grid1(n), dim3(256), 0, g.stream, vs, vd, n);
    else if (ts == GGML_TYPE_I32 && td == GGML_TYPE_I32)
        hipLaunchKernelGGL((k_cpy<int, int>), grid1(n), dim3(256), 0, g.stream, vs, vd, n);
    else
        die("cpy %s -> %s is outside the accelerated path", ggml_type_name(ts), ggml_type_name(td));
    HIP_CHECK(hipGetLastError());
}

void op_get_rows(ggml_tensor *dst) {
    const ggml_tensor *tab = dst->src[0], *ids = dst->src[1];
    BK_ASSERT(ids->type == GGML_TYPE_I32 && is_contig_f32(dst));
    const int64_t N = ids->ne[0], ne0 = tab->ne[0];
    const int *pid = (const int *)dev_ptr(ids);
    float *pd = (float *)dev_ptr(dst);
    Timed tm(GGML_HIP_KCLASS_OTHER, (double)N * ne0 * 5);
    if (qt_of(tab->type) >= 0) {
        const QWeight w = qweight_of(tab);
        hipLaunchKernelGGL(k_get_rows_q, dim3((unsigned)((w.nb + 255) / 256), (unsigned)N), dim3(256), 0, g.stream, w,
                           pid, pd, ne0);
    } else if (kt_of(tab->type) >= 0) {
        dequant_k_rows(kweight_of(tab), pid, N, pd, ne0);
    } else if (tab->type == GGML_TYPE_F16) {
        hipLaunchKernelGGL(k_get_rows<__half>, dim3((unsigned)((ne0 + 255) / 256), (unsigned)N), dim3(256), 0, g.stream,
                           (const char *)dev_ptr(tab), (int64_t)tab->nb[1], pid, pd, ne0);
    } else if (tab->type == GGML_TYPE_F32) {
        hipLaunchKernelGGL(k_get_rows<float>, dim3((unsigned)((ne0 + 255) / 256), (unsigned)N), dim3(256), 0, g.stream,
                           (const char *)dev_ptr(tab), (int64_t)tab->nb[1], pid, pd, ne0);
    } else {
        die("get_rows on %s is outside the accelerated path", ggml_type_name(tab->type));
    }
    HIP_CHECK(hipGetLastError());
}

// GGML_OP_FLASH_ATTN: q [D, N, H, B], k [D, M, Hkv, B], v [M, D, Hkv, B] -> dst [D, N, H, B] f32 in one launch (kernels/flash_attn.h).
// ggml_flash_attn (ggml_core.cpp) has refused every layout the kernels do not take; what is asserted here is that contract.
static inline int prompt_attn_row_bytes(int64_t T);                                                       // plan_shapes.inc
static inline int flash_attn_tile_queries(bool kv_f16, int64_t D, int64_t N, int64_t M, bool aligned16);  // plan_shapes.inc
template <int D, int QR>
static void launch_flash_attn_tile(const FlashAttnArgs &a, dim3 grid, size_t lds) {
    lds_opt_in<k_flash_attn_tile<D, QR>>(lds, FLASH_ATTN_LDS_BYTES);
    hipLaunchKernelGGL((k_flash_attn_tile<D, QR>), grid, dim3(256), lds, g.stream, a);
}
void op_flash_attn(ggml_tensor *dst) {
    const ggml_tensor *q = dst->src[0], *k = dst->src[1], *v = dst->src[2];
    const bool kv16 = k->type == GGML_TYPE_F16;
    const size_t es = kv16 ? 2 : 4;
    BK_ASSERT(is_contig_f32(dst) && k->type == v->type && (kv16 || k->type == GGML_TYPE_F32));
    BK_ASSERT(q->type == GGML_TYPE_F32 || (q->type == GGML_TYPE_F16 && kv16));
    BK_ASSERT(q->nb[0] == ggml_type_size(q->type) && k->nb[0] == es && v->nb[0] == es);
    FlashAttnArgs a;
    a.D = (int)q->ne[0]; a.N = (int)q->ne[1]; a.H = (int)q->ne[2]; a.B = (int)q->ne[3]; a.M = (int)k->ne[1];
    BK_ASSERT(a.D >= 1 && a.D <= FLASH_ATTN_MAX_D && a.N >= 1 && a.M >= a.N && a.M <= FLASH_ATTN_MAX_KEYS);
    BK_ASSERT(k->ne[0] == a.D && v->ne[0] == a.M && v->ne[1] == a.D && k->ne[2] == v->ne[2] && k->ne[2] >= 1 && a.H % k->ne[2] == 0);
    BK_ASSERT(k->ne[3] == a.B && v->ne[3] == a.B);
    BK_ASSERT(dst->ne[0] == a.D && dst->ne[1] == a.N && dst->ne[2] == a.H && dst->ne[3] == a.B);
    const int64_t rows = (int64_t)a.N * a.H * a.B;
    if (rows == 0) return;
    BK_ASSERT(rows < (1ll << 31));
    a.q = dev_ptr(q); a.k = dev_ptr(k); a.v = dev_ptr(v); a.out = (float *)dev_ptr(dst);
    a.q_nb1 = (int64_t)q->nb[1]; a.q_nb2 = (int64_t)q->nb[2]; a.q_nb3 = (int64_t)q->nb[3];
    a.k_nb1 = (int64_t)k->nb[1]; a.k_nb2 = (int64_t)k->nb[2]; a.k_nb3 = (int64_t)k->nb[3];
    a.v_nb1 = (int64_t)v->nb[1]; a.v_nb2 = (int64_t)v->nb[2]; a.v_nb3 = (int64_t)v->nb[3];
    a.r = (int)(a.H / k->ne[2]);
    a.P = a.M - a.N;
    a.masked = dst->op_params[0] != 0;
    a.q16 = q->type == GGML_TYPE_F16;
    a.scale = 1.0f / sqrtf((float)a.D);
    a.kvec = (((uintptr_t)a.k | (uintptr_t)a.k_nb1 | (uintptr_t)a.k_nb2 | (uintptr_t)a.k_nb3) & 15) == 0;
    a.vvec = (((uintptr_t)a.v | (uintptr_t)a.v_nb1 | (uintptr_t)a.v_nb2 | (uintptr_t)a.v_nb3) & 15) == 0;
    a.row_bytes = 0;
    // bytes: q and the result once; per query row the keys it sees (all of them when unmasked), K and V
    const double seen = a.masked ? (double)a.N * (a.P + (a.N + 1) * 0.5) : (double)a.N * a.M;
    Timed tm(GGML_HIP_KCLASS_ATTN, (double)rows * a.D * (ggml_type_size(q->type) + 4.0) + 2.0 * seen * a.D * es * a.H * a.B);
    g.stat_flash_attn_nodes++;
    const int QR = flash_attn_tile_queries(kv16, a.D, a.N, a.M, a.kvec && a.vvec);
    if (QR) {
        a.row_bytes = prompt_attn_row_bytes(a.M);
        const size_t lds = (size_t)QR * a.row_bytes;
        BK_ASSERT(lds <= FLASH_ATTN_LDS_BYTES);
        const int64_t wgs = (int64_t)((a.N + QR - 1) / QR) * a.H * a.B;
        BK_ASSERT(wgs < (1ll << 31));
        const dim3 grid((unsigned)wgs);
        if (QR == 32) {
            if (a.D == 128) launch_flash_attn_tile<128, 32>(a, grid, lds);
            else if (a.D == 64) launch_flash_attn_tile<64, 32>(a, grid, lds);
            else launch_flash_attn_tile<32, 32>(a, grid, lds);
        } else {
            if (a.D == 128) launch_flash_attn_tile<128, 16>(a, grid, lds);
            else if (a.D == 64) launch_flash_attn_tile<64, 16>(a, grid, lds);
            else launch_flash_attn_tile<32, 16>(a, grid, lds);
        }
    } else {
        const size_t lds = FLASH_ROW_RED + (((size_t)a.D * 4 + 15) & ~(size_t)15) + (((size_t)a.M * 4 + 15) & ~(size_t)15);
        BK_ASSERT(lds <= FLASH_ATTN_LDS_BYTES);
        with_bool(kv16, [&](auto KV16) {
            lds_opt_in<k_flash_attn_row<CT(KV16)>>(lds, FLASH_ATTN_LDS_BYTES);
            hipLaunchKernelGGL(k_flash_attn_row<CT(KV16)>, dim3((unsigned)rows), dim3(256), lds, g.stream, a);
        });
    }
    HIP_CHECK(hipGetLastError());
}
