// backend_executor.inc — part of libggml_hip.so's backend translation unit (included by hip_backend.hip, inside its anonymous
// namespace where noted): the graph executor — node-by-node execution, the fused LLaMA plans (plan_*.inc), output mirroring.  Inside the anonymous namespace.
// ---------------------------------------------------------------------------------------------------
// graph executor
// ---------------------------------------------------------------------------------------------------
bool is_view_op(ggml_op op) {
    return op == GGML_OP_NONE || op == GGML_OP_RESHAPE || op == GGML_OP_VIEW || op == GGML_OP_PERMUTE ||
           op == GGML_OP_TRANSPOSE;
}

struct GraphInfo {
    std::vector<int> n_uses;  // consumers per node index
};

int node_index(const ggml_cgraph *gr, const ggml_tensor *t, const std::map<const ggml_tensor *, int> &idx) {
    (void)gr;
    auto it = idx.find(t);
    return it == idx.end() ? -1 : it->second;
}

// The target of a LoRA patch (lora.rs:86-139): the leaf under src0 of an ADD whose src0 is not f32.  Its host bytes are the
// source of truth at compute time — the caller copies the patched result over them afterwards, and a second adapter patches
// the same tensor again — so they are staged raw into the workspace for this graph only (dev_ptr finds them there).  The
// leaf never becomes a persistent or re-laid-out record, and any auto record over its range is dropped: one left behind
// would go stale with the caller's copy, and later graphs that match it by header (weights not offloaded) would read the
// unpatched bytes.  A target the caller already offloaded is not the reference's order (it patches at load, before
// offloading): abort.
void stage_add_target(ggml_tensor *leaf) {
    const uintptr_t p = (uintptr_t)leaf->data;
    const size_t nbytes = ggml_nbytes(leaf);
    for (const Staged &st : g_staged)
        if (st.host == p && st.nbytes == nbytes) return;
    bool offloaded = extra_of(leaf) != nullptr;
    for (auto &kv : g.tensors)
        if (kv.second->host < p + nbytes && p < kv.second->host + std::max<size_t>(kv.second->nbytes, 1)) offloaded = true;
    if (offloaded)
        die("add: tensor '%s' (%s) was offloaded to the device before being patched; LoRA adapters are applied at load time, "
            "before the weights are offloaded",
            leaf->name, ggml_type_name(leaf->type));
    evict_overlapping(g.auto_tensors, p, std::max<size_t>(nbytes, 1));
    char *d = ws_alloc(std::max<size_t>(nbytes, 16));
    h2d_small(d, leaf->data, nbytes);
    g_staged.push_back({p, nbytes, d});
}

void upload_inputs(ggml_cgraph *gr) {
    if (gr->n_nodes == 0) return;
    // the compute context = the arena holding the tensor headers of the graph's nodes
    Arena *r0 = find_arena((uintptr_t)gr->nodes[gr->n_nodes - 1]);
    std::vector<const ggml_tensor *> add_targets;
    for (int i = 0; i < gr->n_nodes; i++) {
        const ggml_tensor *n = gr->nodes[i];
        if (n->op != GGML_OP_ADD || !n->src[0] || n->src[0]->type == GGML_TYPE_F32) continue;
        const ggml_tensor *t = n->src[0];
        while (t->op != GGML_OP_NONE && is_view_op(t->op) && t->src[0]) t = t->src[0];
        if (t->op == GGML_OP_NONE) add_targets.push_back(t);
    }
    for (int i = 0; i < gr->n_leafs; i++) {
        ggml_tensor *leaf = gr->leafs[i];
        if (leaf->data == nullptr) continue;
        if (!add_targets.empty() && std::find(add_targets.begin(), add_targets.end(), leaf) != add_targets.end()) {
            stage_add_target(leaf);
            continue;
        }
        if (extra_of(leaf)) continue;
        const uintptr_t p = (uintptr_t)leaf->data;
        if (DevTensor *e = find_tensor(p)) {
            // auto-uploaded earlier; make sure it still describes this tensor
            if (e->auto_uploaded && (e->host != p || e->nbytes != ggml_nbytes(leaf) || e->type != leaf->type ||
                                     e->owner_hdr != (uintptr_t)leaf)) {
                free_dev_tensor(e);
            } else {
                continue;
            }
        }
        Arena *hdr = find_arena((uintptr_t)leaf);
        const bool per_eval = r0 && hdr == r0;
        if (per_eval) {
            // inputs written by the host before every compute (token ids, scalar constants, test operands)
            const size_t nbytes = ggml_nbytes(leaf);
            if (nbytes == 0) continue;
            h2d_small(dev_ptr(leaf), leaf->data, nbytes);
        } else {
            // persistent tensor (weight / KV memory) that was never offloaded by the caller: upload once
            upload_tensor(leaf->data, leaf, false, /*is_auto=*/true)->owner_hdr = (uintptr_t)leaf;
        }
    }
}

// a node whose result download_outputs copies back to its host data (CPU backend)
bool mirrored_to_host(const ggml_tensor *n) {
    if (n->backend != GGML_BACKEND_CPU || is_view_op(n->op) || n->op == GGML_OP_CPY) return false;
    if (!ggml_is_contiguous(n) || n->data == nullptr) return false;
    return !(extra_of(n) || find_tensor((uintptr_t)n->data));  // else the result aliases a device-resident tensor
}

static inline uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}
void download_outputs(ggml_cgraph *gr) {
    const uint64_t t0 = now_ns();
    bool any = false;
    for (int i = 0; i < gr->n_nodes; i++) {
        ggml_tensor *n = gr->nodes[i];
        if (!mirrored_to_host(n)) continue;
        d2h_queue(n->data, dev_ptr(n), ggml_nbytes(n));
        g.stat_mirror_bytes += ggml_nbytes(n);
        any = true;
    }
    (void)any;
    d2h_finish();
    g.ns_mirror += now_ns() - t0;
}

void invalidate_xf16_if_overwritten_impl(const ggml_tensor *n);
void invalidate_qact_if_overwritten(const ggml_tensor *n) {
    if (g_xi8.valid && n->data != nullptr) {
        const uintptr_t c0 = (uintptr_t)g_xi8.src_data, c1 = c0 + g_xi8.src_bytes;
        const uintptr_t b0 = (uintptr_t)n->data, b1 = b0 + ggml_nbytes(n);
        if (b0 < c1 && c0 < b1) g_xi8.valid = false;
    }
    if (g_xk.valid && n->data != nullptr) {
        const uintptr_t c0 = (uintptr_t)g_xk.src_data, c1 = c0 + g_xk.src_bytes;
        const uintptr_t b0 = (uintptr_t)n->data, b1 = b0 + ggml_nbytes(n);
        if (b0 < c1 && c0 < b1) g_xk.valid = false;
    }
    invalidate_xf16_if_overwritten_impl(n);
    if (!g_qact.valid || n->data == nullptr) return;
    const uintptr_t a0 = (uintptr_t)g_qact.src_data, a1 = a0 + g_qact.src_bytes;
    const uintptr_t b0 = (uintptr_t)n->data, b1 = b0 + ggml_nbytes(n);
    if (b0 < a1 && a0 < b1) g_qact.valid = false;
}
void invalidate_xf16_if_overwritten_impl(const ggml_tensor *n) {
    if (!g_xf16.valid || n->data == nullptr) return;
    const uintptr_t a0 = (uintptr_t)g_xf16.src_data, a1 = a0 + g_xf16.src_bytes;
    const uintptr_t b0 = (uintptr_t)n->data, b1 = b0 + ggml_nbytes(n);
    if (b0 < a1 && a0 < b1) g_xf16.valid = false;
}

// the fused LLaMA plans, one concern per file (plan_shapes.inc says which); finish_pending is plan_run.inc's
#include "plan_shapes.inc"
#include "plan_match.inc"
#include "plan_build.inc"
#include "plan_decode.inc"
#include "plan_prompt.inc"
#include "plan_run.inc"
#include "plan_pool.inc"
#include "plan_pack.inc"

void execute_graph(ggml_cgraph *gr) {
    ensure_init();
    finish_pending();
    ws_reset();
    g_qact.valid = false;
    g_xf16.valid = false;
    g_xi8.valid = false;
    g_xk.valid = false;
    if (try_decode_plan(gr)) return;  // single-token LLaMA decode: fused launches + hipGraph replay
    // node by node: no hit check was reached — a token that ran ahead is taken back now (this graph may write the cache rows it
    // wrote), and a last evaluated token that sits in a result set 1 goes into its graph's own nodes
    spec_cancel();
    res_settle();
    g.stat_generic_graphs++;
    upload_inputs(gr);

    std::map<const ggml_tensor *, int> idx;
    std::vector<int> uses(gr->n_nodes, 0);
    for (int i = 0; i < gr->n_nodes; i++) idx[gr->nodes[i]] = i;
    for (int i = 0; i < gr->n_nodes; i++)
        for (int s = 0; s < GGML_MAX_SRC; s++)
            if (gr->nodes[i]->src[s]) {
                int j = node_index(gr, gr->nodes[i]->src[s], idx);
                if (j >= 0) uses[j]++;
            }
    std::vector<char> done(gr->n_nodes, 0);
    const bool fuse = g.opt_fuse != 0;
    // silu(a) whose only consumer is a later mul(silu(a), b) — the FFN gate; the reference's build order puts the
    // w3 mat-mul between the two (nodes: w1·x, silu, w3·x, mul), so the pair is not adjacent: the silu is deferred
    // and executed fused when its mul comes up.  That reads a when the mul runs, not when the silu would have: a node
    // in between whose result overlaps a's bytes (an in-place op on a, a cpy into it) would change what the silu sees,
    // so such a silu is not deferred and runs in its own place.
    std::vector<int> deferred_silu(gr->n_nodes, -1);  // index of the mul that will run it
    auto written_between = [&](const ggml_tensor *t, int i, int j) {  // does a node of (i, j) write bytes of t?
        const uintptr_t a0 = (uintptr_t)t->data, a1 = a0 + ggml_nbytes(t);
        for (int k = i + 1; k < j; k++) {
            const ggml_tensor *w = gr->nodes[k];
            if (is_view_op(w->op) || w->data == nullptr) continue;
            const uintptr_t b0 = (uintptr_t)w->data, b1 = b0 + ggml_nbytes(w);
            if (b0 < a1 && a0 < b1) return true;
        }
        return false;
    };
    if (fuse) {
        for (int j = 0; j < gr->n_nodes; j++) {
            ggml_tensor *mu = gr->nodes[j];
            if (mu->op != GGML_OP_MUL || !mu->src[0] || mu->src[0]->op != GGML_OP_UNARY) continue;
            const int i = node_index(gr, mu->src[0], idx);
            ggml_tensor *un = mu->src[0];
            if (i < 0 || i >= j || uses[i] != 1 || un->op_params[0] != GGML_UNARY_OP_SILU) continue;
            if (!is_contig_f32(un->src[0]) || !is_contig_f32(mu->src[1]) || !is_contig_f32(mu) ||
                ggml_nelements(mu->src[1]) != ggml_nelements(un) || ggml_nelements(mu) != ggml_nelements(un))
                continue;
            if (written_between(un->src[0], i, j)) continue;
            deferred_silu[i] = j;
        }
    }

    for (int i = 0; i < gr->n_nodes; i++) {
        ggml_tensor *n = gr->nodes[i];
        if (done[i] || is_view_op(n->op)) continue;
        invalidate_qact_if_overwritten(n);
        ggml_tensor *next = i + 1 < gr->n_nodes ? gr->nodes[i + 1] : nullptr;
        switch (n->op) {
            case GGML_OP_GET_ROWS: op_get_rows(n); break;
            case GGML_OP_RMS_NORM: {
                // fuse the broadcast multiply by the norm weight that follows (llama lib.rs:183-186)
                if (fuse && next && next->op == GGML_OP_MUL && next->src[0] == n && uses[i] == 1 && !done[i + 1] &&
                    is_contig_f32(next->src[1]) && ggml_nelements(next->src[1]) == n->ne[0] && next->nb[0] == 4) {
                    invalidate_qact_if_overwritten(next);
                    op_rms_norm(n, next->src[1], next);
                    done[i + 1] = 1;
                } else {
                    op_rms_norm(n, nullptr, n);
                }
            } break;
            case GGML_OP_NORM: op_norm(n); break;
            case GGML_OP_ADD: {
                if (n->src[0]->type == GGML_TYPE_F32)
                    op_bin(n, BIN_ADD);
                else
                    op_add_lowp(n);  // W + s·BA of a LoRA patch: requantizing add (kernels/lora.h)
            } break;
            case GGML_OP_MUL: {
                const int si = n->src[0] && n->src[0]->op == GGML_OP_UNARY ? node_index(gr, n->src[0], idx) : -1;
                if (si >= 0 && deferred_silu[si] == i)
                    op_unary(n->src[0], n->src[1], n);  // silu(a) * b in one pass
                else
                    op_bin(n, BIN_MUL);
            } break;
            case GGML_OP_REPEAT: op_bin(n, BIN_REPEAT); break;
            case GGML_OP_UNARY: {
                if (deferred_silu[i] >= 0) break;  // runs fused with its mul
                if (fuse && n->op_params[0] == GGML_UNARY_OP_SILU && next && next->op == GGML_OP_MUL &&
                    next->src[0] == n && uses[i] == 1 && !done[i + 1] && is_contig_f32(next->src[1]) &&
                    ggml_nelements(next->src[1]) == ggml_nelements(n) && is_contig_f32(next)) {
                    invalidate_qact_if_overwritten(next);
                    op_unary(n, next->src[1], next);
                    done[i + 1] = 1;
                } else {
                    op_unary(n, nullptr, n);
                }
            } break;
            case GGML_OP_MUL_MAT: op_mul_mat(n); break;
            case GGML_OP_SCALE: {
                // fuse scale -> diag_mask_inf -> soft_max when chained in place (llama lib.rs:268-281)
                ggml_tensor *n1 = next, *n2 = i + 2 < gr->n_nodes ? gr->nodes[i + 2] : nullptr;
                ggml_tensor *n3 = i + 3 < gr->n_nodes ? gr->nodes[i + 3] : nullptr;
                if (fuse && n1 && n2 && n1->op == GGML_OP_DIAG_MASK_INF && n1->src[0] == n && n2->op == GGML_OP_SOFT_MAX &&
                    n2->src[0] == n1 && uses[i] == 1 && uses[i + 1] == 1 && n->data == n->src[0]->data &&
                    n1->data == n->data && n2->data == n->data && is_contig_f32(n)) {
                    op_scale_mask_softmax(n->src[0], n->src[1], (int)n1->op_params[0], n2);
                    done[i + 1] = done[i + 2] = 1;
                } else if (fuse && n1 && n2 && n3 && n1->op == GGML_OP_ALIBI && n1->src[0] == n &&
                           n2->op == GGML_OP_DIAG_MASK_INF && n2->src[0] == n1 && n3->op == GGML_OP_SOFT_MAX &&
                           n3->src[0] == n2 && uses[i] == 1 && uses[i + 1] == 1 && uses[i + 2] == 1 &&
                           !mirrored_to_host(n) && !mirrored_to_host(n1) && !mirrored_to_host(n2) &&
                           is_contig_f32(n->src[0]) && is_contig_f32(n3) && ggml_nelements(n3) == ggml_nelements(n) &&
                           n3->ne[0] == n->src[0]->ne[0] && n3->ne[1] == n->src[0]->ne[1] && n->src[0]->ne[3] == 1 &&
                           n->src[0]->ne[2] == n1->op_params[1]) {
                    // BLOOM / MPT (bloom lib.rs:233-246, mpt lib.rs:176-183), built out of place: S = scale(KQ), A = alibi
                    // view of S, M = diag_mask_inf(A), P = soft_max(M) (any step may also be in place).  S, A and M have no
                    // other reader and are not mirrored to the host, so they need not be written: one launch reads KQ and
                    // writes P.
                    invalidate_qact_if_overwritten(n3);
                    op_scale_alibi_mask_softmax(n->src[0], n->src[1], n1, (int)n2->op_params[0], n3);
                    done[i + 1] = done[i + 2] = done[i + 3] = 1;
                    g.stat_alibi_fused++;
                } else {
                    op_scale(n);
                }
            } break;
            case GGML_OP_DIAG_MASK_INF: op_diag_mask_inf(n); break;
            case GGML_OP_SOFT_MAX: op_soft_max(n); break;
            case GGML_OP_ALIBI: op_alibi(n); break;
            case GGML_OP_ROPE: op_rope(n); break;
            case GGML_OP_FLASH_ATTN: op_flash_attn(n); break;
            case GGML_OP_CPY: op_cpy(n->src[0], n->src[1]); break;
            case GGML_OP_CONT:
            case GGML_OP_DUP: op_cpy(n->src[0], n); break;
            default:
                die("op %s (node '%s') is outside the accelerated path and this library has no CPU fallback",
                    ggml_op_name(n->op), n->name);
        }
    }
    download_outputs(gr);
}
