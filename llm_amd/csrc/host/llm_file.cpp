// llm_file.cpp — the host mirror's loaders: the GGML / GGMF / GGJT container reader (crates/ggml/src/format/loader.rs:160-281) with
// llm_llama_load on top of it, and llm::load::<Llama> with LoRA adapters (llm_llama_load_lora).  The model itself is made by
// llm_llama_new (llm_host.cpp) from the tensor descriptors read here.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <map>
#include <set>

#include "llm_session.hpp"

// ---------------------------------------------------------------------------------------------------------------
// GGML / GGMF / GGJT container reader (crates/ggml/src/format/loader.rs:160-281), tensor data left in the mapping
// ---------------------------------------------------------------------------------------------------------------
struct llm_ggml_file {
    int fd = -1;
    const uint8_t *base = nullptr;
    size_t size = 0;
    bool owned = false;  // base is a heap buffer the file was read into (llm_llama_load_lora: weights are patched in place)
    int container = 0, version = 0;
    llm_llama_hparams hp{};
    int32_t lora_r = 0, lora_alpha = 0;  // ggla (LoraParameters, crates/llm-base/src/lora.rs:28-34)
    struct Tok {
        const char *p;
        uint32_t len;
        float score;
    };
    std::vector<Tok> vocab;
    struct Ten {
        std::string name;
        int32_t type, n_dims;
        int64_t ne[2];
        size_t offset;
    };
    std::vector<Ten> tensors;
};

namespace {
struct Cursor {
    const uint8_t *p, *end;
    bool ok = true;
    uint32_t u32() {
        uint32_t v = 0;
        if ((size_t)(end - p) < 4) {
            ok = false;
            return v;
        }
        memcpy(&v, p, 4);
        p += 4;
        return v;
    }
    int32_t i32() { return (int32_t)u32(); }
    float f32() {
        const uint32_t u = u32();
        float v;
        memcpy(&v, &u, 4);
        return v;
    }
    const uint8_t *bytes(size_t n) {
        if ((size_t)(end - p) < n) {
            ok = false;
            return nullptr;
        }
        const uint8_t *r = p;
        p += n;
        return r;
    }
};
size_t ggml_file_type_size(int32_t t) {  // bytes per block; blck via ggml_blck_size
    return ggml_type_size((ggml_type)t);
}

llm_ggml_file *ggml_file_open(const char *path, bool owned) {
    auto fail = [&](llm_ggml_file *f, const char *why) -> llm_ggml_file * {
        fprintf(stderr, "llm_ggml_file_open(%s): %s\n", path, why);
        if (f) llm_ggml_file_close(f);
        return nullptr;
    };
    llm_ggml_file *f = new llm_ggml_file();
    f->fd = open(path, O_RDONLY);
    if (f->fd < 0) return fail(f, "cannot open file");
    struct stat st;
    if (fstat(f->fd, &st) != 0 || st.st_size < 8) return fail(f, "cannot stat file / file too small");
    f->size = (size_t)st.st_size;
    if (owned) {  // prefer_mmap is off when adapters are given (loader.rs:485-486): the tensors live in a writable copy
        uint8_t *buf = (uint8_t *)malloc(f->size);
        if (!buf) return fail(f, "cannot allocate the model buffer");
        f->base = buf;
        f->owned = true;
        size_t off = 0;
        while (off < f->size) {
            const ssize_t r = pread(f->fd, buf + off, std::min<size_t>(f->size - off, (size_t)1 << 30), (off_t)off);
            if (r <= 0) return fail(f, "read failed");
            off += (size_t)r;
        }
    } else {
        void *m = mmap(nullptr, f->size, PROT_READ, MAP_SHARED, f->fd, 0);
        if (m == MAP_FAILED) return fail(f, "mmap failed");
        f->base = (const uint8_t *)m;
    }
    Cursor c{f->base, f->base + f->size};
    // ContainerType::read (crates/ggml/src/lib.rs:58-84)
    const uint32_t magic = c.u32();
    if (magic == 0x67676d6cu) {  // 'ggml': unversioned
        f->container = 0;
    } else if (magic == 0x67676d66u || magic == 0x67676a74u || magic == 0x67676c61u) {
        f->container = magic == 0x67676d66u ? 1 : magic == 0x67676a74u ? 2 : 3;
        f->version = (int)c.u32();
    } else {
        return fail(f, "LoadError::InvalidMagic");
    }
    const bool ok_version = f->container == 0 || (f->container == 1 && f->version == 1) ||
                            (f->container == 2 && f->version >= 1 && f->version <= 3) ||
                            (f->container == 3 && f->version == 1);
    if (!ok_version) return fail(f, "LoadError::InvalidFormatVersion");
    if (f->container == 3) {
        // a LoRA adapter: LoraParameters { r, alpha } and no vocabulary (lora.rs:28-52); tensor data 32-byte aligned
        f->lora_r = c.i32();
        f->lora_alpha = c.i32();
        if (!c.ok) return fail(f, "LoadError: bad hyperparameters");
    } else {
        // LLaMA hyperparameters (models/llama/src/lib.rs:425-447)
        f->hp.n_vocab = c.i32();
        f->hp.n_embd = c.i32();
        f->hp.n_mult = c.i32();
        f->hp.n_head = c.i32();
        f->hp.n_layer = c.i32();
        f->hp.n_rot = c.i32();
        f->hp.file_type = c.i32();
        f->hp.n_head_kv = f->hp.n_head;
        if (!c.ok || f->hp.n_vocab < 0 || f->hp.n_embd <= 0 || f->hp.n_head <= 0 || f->hp.n_layer <= 0)
            return fail(f, "LoadError: bad hyperparameters");
    }
    for (int i = 0; i < f->hp.n_vocab; i++) {  // loader.rs:187-203
        const uint32_t len = c.u32();
        const uint8_t *tok = c.bytes(len);
        float score = 0.0f;
        if (f->container == 1 || f->container == 2) score = c.f32();
        if (!c.ok) return fail(f, "LoadError: truncated vocabulary");
        f->vocab.push_back({(const char *)tok, len, score});
    }
    const bool align = f->container >= 2;  // loader.rs:206-212
    while (c.p < c.end) {                  // load_weights, loader.rs:219-281
        llm_ggml_file::Ten t;
        t.n_dims = c.i32();
        const int32_t name_len = c.i32();
        const uint32_t ftype = c.u32();
        if (!c.ok || t.n_dims < 1 || t.n_dims > 2 || name_len < 0) return fail(f, "LoadError::InvariantBroken (n_dims <= 2)");
        t.ne[0] = t.ne[1] = 1;
        int64_t n_elements = 1;
        for (int i = 0; i < t.n_dims; i++) {
            t.ne[i] = c.i32();
            if (t.ne[i] <= 0) return fail(f, "LoadError: bad tensor dimension");
            n_elements *= t.ne[i];
        }
        const uint8_t *nm = c.bytes((size_t)name_len);
        if (!c.ok) return fail(f, "LoadError: truncated tensor header");
        t.name.assign((const char *)nm, (size_t)name_len);
        if (ftype >= GGML_TYPE_COUNT || ggml_blck_size((ggml_type)ftype) == 0 || ggml_file_type_size((int32_t)ftype) == 0)
            return fail(f, "LoadError::UnsupportedElementType");
        t.type = (int32_t)ftype;
        if ((t.type == GGML_TYPE_Q4_0 || t.type == GGML_TYPE_Q4_1) && t.ne[0] % 64 != 0)
            return fail(f, "LoadError::InvariantBroken (dims[0] % 64 == 0)");
        size_t off = (size_t)(c.p - f->base);
        if (align) off = (off + 31) & ~(size_t)31;
        const size_t n_bytes = ggml_file_type_size(t.type) * (size_t)n_elements / (size_t)ggml_blck_size((ggml_type)t.type);
        if (off + n_bytes > f->size) return fail(f, "LoadError: tensor data past the end of the file");
        t.offset = off;
        f->tensors.push_back(t);
        c.p = f->base + off + n_bytes;
    }
    return f;
}
// Model::new over an opened container: its tensors as descriptors into the mapping, which the model keeps alive
llm_model *model_of_file(llm_ggml_file *f, const llm_model_params *params) {
    std::vector<llm_tensor_desc> descs(f->tensors.size());
    for (size_t i = 0; i < descs.size(); i++) llm_ggml_file_tensor(f, (int)i, &descs[i]);
    llm_model *m = llm_llama_new(&f->hp, params, descs.data(), (int)descs.size());
    m->file = f;
    return m;
}

// llm::load::<Llama> with ModelParameters::lora_adapters (crates/llm-base/src/loader.rs:486-531, 651-670; lora.rs:71-141)
struct LoraFile {
    llm_ggml_file *f = nullptr;
    std::string path;
    float scaling = 1.0f;
    std::map<std::string, int> tensors;  // name -> index in f->tensors
    std::set<std::string> to_patch;      // every tensor name minus its last '.'-component
};
std::atomic<int64_t> g_lora_ns[4] = {};  // [0] model read, [1] adapter open, [2] patching (all of it), [3] copies over W
double lora_now_ns() {
    return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// one LoraAdapter::patch: out = add(W, [scale](mul_mat(A, B), s)) in a fresh CPU context sized by lora.rs's formula,
// computed, then copied over W.  Returns false after printing a LoadError-style message.
bool lora_patch(const LoraFile &ad, const llm_ggml_file::Ten &wi, uint8_t *wdata) {
    auto info = [&](const std::string &n) -> const llm_ggml_file::Ten * {
        auto it = ad.tensors.find(n);
        if (it == ad.tensors.end()) {
            fprintf(stderr, "LoadError::UnknownTensor { tensor_name: \"%s\", path: \"%s\" }\n", n.c_str(), ad.path.c_str());
            return nullptr;
        }
        return &ad.f->tensors[(size_t)it->second];
    };
    const llm_ggml_file::Ten *ai = info(wi.name + ".loraA"), *bi = info(wi.name + ".loraB");
    if (!ai || !bi) return false;
    auto data_size = [](int32_t type, int64_t n) {
        return ggml_type_size((ggml_type)type) * (size_t)n / (size_t)ggml_blck_size((ggml_type)type);
    };
    const size_t header = sizeof(ggml_tensor) + sizeof(ggml_object);
    const int64_t nw = wi.ne[0] * wi.ne[1];
    const bool must_scale = ad.scaling != 1.0f;
    const size_t ba_size = header + data_size(ai->type, nw);  // (the element type of A, as the reference writes it)
    size_t ctx_size = header + data_size(ai->type, ai->ne[0] * ai->ne[1]) + header + data_size(bi->type, bi->ne[0] * bi->ne[1]) +
                      header + data_size(wi.type, nw) + ba_size;
    if (must_scale) ctx_size += header + data_size(GGML_TYPE_F32, nw) + ba_size;
    ctx_size += ctx_size / 20;
    // The formula leaves the graph (ggml_graph_overhead) to the 5 %, and counts ba at A's element size though mul_mat
    // makes it f32: small tensors, and an f16 A with scaling 1, do not fit, where the reference's ggml would abort.  The
    // context is only scratch for this graph, so it is raised to what the graph takes (the results do not depend on it).
    auto al = [](size_t x) { return (x + 15) & ~(size_t)15; };
    const size_t need = 6 * ggml_tensor_overhead() + ggml_graph_overhead() + al(data_size(ai->type, ai->ne[0] * ai->ne[1])) +
                        al(data_size(bi->type, bi->ne[0] * bi->ne[1])) + 2 * al(data_size(GGML_TYPE_F32, nw)) + 16 +
                        al(data_size(wi.type, nw)) + 4096;
    ctx_size = std::max(ctx_size, need);
    ggml_init_params ip = {ctx_size, nullptr, false};
    ggml_context *pc = ggml_init(ip);
    ggml_init_params wp = {ggml_tensor_overhead(), nullptr, true};
    ggml_context *wc = ggml_init(wp);  // the header of the target: its data is the model's buffer
    auto load = [&](const llm_ggml_file::Ten *t) {
        ggml_tensor *x = ggml_new_tensor_2d(pc, (ggml_type)t->type, t->ne[0], t->ne[1]);
        memcpy(x->data, ad.f->base + t->offset, ggml_nbytes(x));
        return x;
    };
    ggml_tensor *a = load(ai), *b = load(bi);
    ggml_tensor *w = ggml_new_tensor_2d(wc, (ggml_type)wi.type, wi.ne[0], wi.ne[1]);
    w->data = wdata;
    ggml_cgraph *gf = ggml_new_graph(pc);
    ggml_tensor *ba = ggml_mul_mat(pc, a, b);
    if (must_scale) ba = ggml_scale(pc, ba, ggml_new_f32(pc, ad.scaling));
    ggml_tensor *out = ggml_add(pc, w, ba);
    ggml_build_forward_expand(gf, out);
    ggml_cplan plan = ggml_graph_plan(gf, 8);
    std::vector<uint8_t> work(plan.work_size);
    plan.work_data = work.empty() ? nullptr : work.data();
    ggml_graph_compute(gf, &plan);
    const double t = lora_now_ns();
    memcpy(wdata, out->data, ggml_nbytes(w));
    g_lora_ns[3] += (int64_t)(lora_now_ns() - t);
    ggml_free(wc);
    ggml_free(pc);
    return true;
}
}  // namespace

extern "C" {

llm_ggml_file *llm_ggml_file_open(const char *path) { return ggml_file_open(path, false); }
void llm_ggml_file_close(llm_ggml_file *f) {
    if (!f) return;
    if (f->base && f->owned) free((void *)f->base);
    else if (f->base) munmap((void *)f->base, f->size);
    if (f->fd >= 0) close(f->fd);
    delete f;
}
int llm_ggml_file_lora(const llm_ggml_file *f, int *r, int *alpha) {
    if (f->container != 3) return -1;
    if (r) *r = f->lora_r;
    if (alpha) *alpha = f->lora_alpha;
    return 0;
}
void llm_ggml_file_info(const llm_ggml_file *f, int *container, int *version, llm_llama_hparams *hp, int *n_tensors,
                        int *n_vocab_entries) {
    if (container) *container = f->container;
    if (version) *version = f->version;
    if (hp) *hp = f->hp;
    if (n_tensors) *n_tensors = (int)f->tensors.size();
    if (n_vocab_entries) *n_vocab_entries = (int)f->vocab.size();
}
int llm_ggml_file_tensor(const llm_ggml_file *f, int i, llm_tensor_desc *d) {
    if (i < 0 || i >= (int)f->tensors.size()) return -1;
    const auto &t = f->tensors[(size_t)i];
    d->name = t.name.c_str();
    d->type = t.type;
    d->n_dims = t.n_dims;
    d->ne[0] = t.ne[0];
    d->ne[1] = t.ne[1];
    d->data = (void *)(f->base + t.offset);
    return 0;
}
int llm_ggml_file_vocab(const llm_ggml_file *f, int i, char *buf, int cap, float *score) {
    if (i < 0 || i >= (int)f->vocab.size()) return -1;
    const auto &t = f->vocab[(size_t)i];
    if (buf && cap > 0) memcpy(buf, t.p, std::min<size_t>((size_t)cap, t.len));
    if (score) *score = t.score;
    return (int)t.len;
}
llm_model *llm_llama_load(const char *path, const llm_model_params *params) {
    llm_ggml_file *f = llm_ggml_file_open(path);
    return f ? model_of_file(f, params) : nullptr;
}
llm_model *llm_llama_load_lora(const char *path, const llm_model_params *params, const char *const *lora_paths, int n_lora) {
    std::vector<LoraFile> ads((size_t)std::max(n_lora, 0));
    auto cleanup = [&](llm_ggml_file *f) -> llm_model * {
        for (auto &ad : ads)
            if (ad.f) llm_ggml_file_close(ad.f);
        if (f) llm_ggml_file_close(f);
        return nullptr;
    };
    double t0 = lora_now_ns();
    for (int i = 0; i < n_lora; i++) {  // every adapter is opened and read before the model (loader.rs:494-528)
        LoraFile &ad = ads[(size_t)i];
        ad.path = lora_paths[i];
        ad.f = llm_ggml_file_open(lora_paths[i]);
        if (!ad.f) return cleanup(nullptr);
        int r = 0, alpha = 0;
        if (llm_ggml_file_lora(ad.f, &r, &alpha) != 0) {
            fprintf(stderr, "llm_llama_load_lora(%s): LoadError::InvalidMagic (not a ggla LoRA adapter)\n", lora_paths[i]);
            return cleanup(nullptr);
        }
        ad.scaling = (float)alpha / (float)r;  // LoraParameters::calculate_scaling
        for (size_t k = 0; k < ad.f->tensors.size(); k++) {
            const std::string &n = ad.f->tensors[k].name;
            ad.tensors[n] = (int)k;
            const size_t dot = n.rfind('.');
            if (dot != std::string::npos) ad.to_patch.insert(n.substr(0, dot));
        }
    }
    const double t1 = lora_now_ns();
    g_lora_ns[1] += (int64_t)(t1 - t0);
    llm_ggml_file *f = ggml_file_open(path, /*owned=*/true);
    if (!f) return cleanup(nullptr);
    const double t2 = lora_now_ns();
    g_lora_ns[0] += (int64_t)(t2 - t1);
    for (const auto &wi : f->tensors)
        for (const LoraFile &ad : ads) {  // every adapter, in the order given (loader.rs:660-667)
            if (!ad.to_patch.count(wi.name)) continue;
            if (!lora_patch(ad, wi, (uint8_t *)f->base + wi.offset)) return cleanup(f);
        }
    g_lora_ns[2] += (int64_t)(lora_now_ns() - t2);
    for (auto &ad : ads) llm_ggml_file_close(ad.f);
    ads.clear();
    return model_of_file(f, params);
}
void llm_lora_timing(double *out4, int reset) {
    for (int i = 0; i < 4; i++) out4[i] = (double)g_lora_ns[i].load();
    if (reset) for (int i = 0; i < 4; i++) g_lora_ns[i].store(0);
}

}  // extern "C"
