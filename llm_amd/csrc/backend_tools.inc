// backend_tools.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip, inside its anonymous
// namespace where noted): measurement — the launch probe, counters, timeline read-back, version.  At file scope.
//
// Launch-floor probe (tests/tools/launch_probe.py): a linear hipGraph of `n_launch` launches of a kernel that does
// nothing but stamp the 100 MHz wall clock — at its very first instruction, again once its LAST kernel argument has
// arrived, and at its end — with the launch shape of the decode mat-vecs (threads per workgroup, dynamic LDS, size
// of the kernarg segment).  Separates what a kernel boundary costs by itself, and how long the kernel arguments
// take to arrive, from what the mat-vec kernels add.  out[0] = us per launch (HIP events around `replays` replays),
// out[1] = us from one launch's end stamp to the next launch's first instruction, out[2] = us first instruction ->
// last kernel argument usable (workgroup 0 of each launch).
namespace {
template <int NARG>
struct EmptyArgs {
    long long *ts;
    int idx;
    int pad[(NARG - 12) / 4];
};
template <int NARG>
__global__ void __launch_bounds__(1024) k_empty(const EmptyArgs<NARG> a, int last_arg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    long long t0;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0));
    const int v = a.pad[(NARG - 12) / 4 - 1] + last_arg;  // the far end of the kernarg segment
    long long t1 = v != 0x7fffffff ? (long long)wall_clock64() : 0;
    if (v == 0x12345678) smem[threadIdx.x] = 1;  // keeps the dynamic LDS allocation referenced
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        a.ts[a.idx * 4] = t0;
        a.ts[a.idx * 4 + 1] = t1;
        a.ts[a.idx * 4 + 2] = (long long)wall_clock64();
    }
}
template <int NARG>
void empty_launch(int wgs, int threads, int lds, long long *ts, int idx) {
    EmptyArgs<NARG> a;
    memset(&a, 0, sizeof(a));
    a.ts = ts;
    a.idx = idx;
    lds_opt_in<k_empty<NARG>>((size_t)lds, 160 * 1024);
    hipLaunchKernelGGL(k_empty<NARG>, dim3(wgs), dim3(threads), (size_t)lds, g.stream, a, 0);
}
}  // namespace
extern "C" {
int ggml_hip_bench_empty(int wgs, int threads, int lds_bytes, int kernarg_bytes, int n_launch, int replays, double *out) {
    SlotLock lk;
    ensure_init();
    if (n_launch < 2 || n_launch > 512 || replays < 1 || threads < 64 || threads > 1024 || lds_bytes > 160 * 1024) return -1;
    long long *ts = nullptr;
    HIP_CHECK(hipMalloc((void **)&ts, (size_t)n_launch * 32));
    HIP_CHECK(hipMemsetAsync(ts, 0, (size_t)n_launch * 32, g.stream));
    hipGraph_t gr = nullptr;
    hipGraphExec_t ex = nullptr;
    HIP_CHECK(hipStreamBeginCapture(g.stream, hipStreamCaptureModeThreadLocal));
    for (int i = 0; i < n_launch; i++) {
        if (kernarg_bytes <= 64) empty_launch<64>(wgs, threads, lds_bytes, ts, i);
        else if (kernarg_bytes <= 192) empty_launch<192>(wgs, threads, lds_bytes, ts, i);
        else empty_launch<448>(wgs, threads, lds_bytes, ts, i);
    }
    HIP_CHECK(hipStreamEndCapture(g.stream, &gr));
    HIP_CHECK(hipGraphInstantiate(&ex, gr, nullptr, nullptr, 0));
    HIP_CHECK(hipGraphLaunch(ex, g.stream));
    hipEvent_t a, b;
    HIP_CHECK(hipEventCreate(&a));
    HIP_CHECK(hipEventCreate(&b));
    HIP_CHECK(hipEventRecord(a, g.stream));
    for (int i = 0; i < replays; i++) HIP_CHECK(hipGraphLaunch(ex, g.stream));
    HIP_CHECK(hipEventRecord(b, g.stream));
    HIP_CHECK(hipStreamSynchronize(g.stream));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    std::vector<long long> h((size_t)n_launch * 4);
    HIP_CHECK(hipMemcpy(h.data(), ts, (size_t)n_launch * 32, hipMemcpyDeviceToHost));
    double gap = 0, karg = 0;
    for (int i = 1; i < n_launch; i++) {
        gap += (double)(h[i * 4] - h[(i - 1) * 4 + 2]) / 100.0;
        karg += (double)(h[i * 4 + 1] - h[i * 4]) / 100.0;
    }
    out[0] = (double)ms * 1e3 / ((double)n_launch * replays);
    out[1] = gap / (n_launch - 1);
    out[2] = karg / (n_launch - 1);
    HIP_CHECK(hipEventDestroy(a));
    HIP_CHECK(hipEventDestroy(b));
    HIP_CHECK(hipGraphExecDestroy(ex));
    HIP_CHECK(hipGraphDestroy(gr));
    HIP_CHECK(hipFree(ts));
    return 0;
}

int64_t ggml_hip_get_stat(const char *key) {
    SlotLock lk;
    for (const StatRow &c : g_counters)  // the plain counters (backend_state.inc); the rest is computed here
        if (!strcmp(c.key, key)) return (int64_t)(g.*c.field);
    const std::string k(key);
    if (k == "w16_bytes") return (int64_t)g.w16_bytes;  // HBM held by resident f16 weight copies
    if (k.rfind("mmq_launches_", 0) == 0) {                 // prompt-GEMM launches by kernel since library load
        static const char *names[Backend::MMQ_K_COUNT] = {"plain", "dma_p8", "w16_p8", "w16_256", "i8"};
        for (int i = 0; i < Backend::MMQ_K_COUNT; i++)
            if (k.substr(13) == names[i]) return (int64_t)g.stat_mmq[i];
        return -1;
    }
    if (k == "graph_replays") {
        int64_t n = 0;
        for (auto *p : g_plans) n += (int64_t)p->replays;
        return n;
    }
    if (k == "plans") return (int64_t)g_plans.size();
    if (k == "num_cus") {  // workgroups of a full-chip mat-vec launch (k_mmvq_big, k_mmvq_kbig)
        ensure_init();
        return (int64_t)g.num_cus;
    }
    if (k == "fused_attn_timeouts") {  // attention workgroups of k_qkv_attn that gave up waiting (must stay 0)
        int64_t n = (int64_t)g.stat_fused_timeouts;  // tokens the host saw the error word for (re-run or fatal) + a word still set
        if (g.inited) HIP_CHECK(hipStreamSynchronize(g.stream));
        if (g.ferr_pin) n += *(volatile unsigned *)g.ferr_pin;
        return n;
    }
    if (k == "peak_concurrent_calls") return (int64_t)g_calls_inside_peak.load();  // threads that were inside entry points (on different slots) at once
    return -1;
}
size_t ggml_hip_read_timeline(int64_t *dst, size_t max_records) {
    SlotLock lk;
    if (!g.timeline) return 0;
    const size_t n = std::min(max_records, g.timeline_bytes / 64);
    HIP_CHECK(hipStreamSynchronize(g.stream));
    HIP_CHECK(hipMemcpy(dst, g.timeline, n * 64, hipMemcpyDeviceToHost));
    return n;
}
const char *ggml_hip_version(void) { return "libggml_hip 0.1 (gfx950)"; }

}  // extern "C"
