// C-ABI of the DiT training step (include/gtav_amd.h): forward with saved activations, backward, AdamW, optimizer state.
#include "api_internal.h"

#include <algorithm>

static int g_dw_grouped = GTAV_ENV_INT("GTAV_DW_GROUPED", 1);   // experiments build: 0 = one launch per weight gradient (A/B runs)
static int g_fuse_gelu_fwd = GTAV_ENV_INT("GTAV_FUSE_GELU_FWD", 1); // experiments build: 0 = h = GELU(u) by the flat elementwise kernel behind fc1 (A/B runs)
static int g_fuse_gelu = GTAV_ENV_INT("GTAV_FUSE_GELU_BWD", 1); // experiments build: 0 = gelu_bwd and the fc1 bias column sums as two launches (A/B runs)
static int g_fuse_ln = GTAV_ENV_INT("GTAV_FUSE_LN_BWD", 1);     // experiments build: 0 = ln_mod_bwd and frame_reduce_ln as two launches (A/B runs)
static int g_fuse_gate = GTAV_ENV_INT("GTAV_FUSE_GATE", 1);     // experiments build: 0 = gate_bwd, frame_reduce_gate and the bias column sums as three launches (A/B runs)
static int g_dw_tn = GTAV_ENV_INT("GTAV_DW_TN", 1);             // experiments build: 0 = transposed operand copies in front of the grouped launch (A/B runs)

// The training step serves windows of at most 8 frames unless the caller opted in to longer ones (gtav_dit_train_allow_window): refused by name before anything on
// the handle is allocated or changed.
static int train_window_ok(const gtav_dit* h) {
    if (h->tr.window > 8) {
        GTAV_REQUIRE(h->maxT <= h->tr.window, "train_enable: gtav_dit_train_allow_window allowed training windows of at most %d frames on this handle; it was created "
                     "with max_frames=%d", h->tr.window, h->maxT);
        return 0;
    }
    GTAV_REQUIRE(h->maxT <= 8, "train_enable: training is implemented for windows of at most 8 frames (the backward temporal attention and the adaLN-gradient "
                 "reduction are sized for it); this handle was created with max_frames=%d", h->maxT);
    return 0;
}

// The slots whose gradients the backward pass writes, by name, once (after the gradients were laid out): a name that is not a trainable slot is refused here
// instead of becoming a write through a null pointer in the middle of a step.
static int train_linear(gtav_dit* h, const std::string& n, gtav_dit::Train::Linear* out, bool bias = true) {
    out->w = h->wt.find(n + ".weight");
    out->b = bias ? h->wt.find(n + ".bias") : nullptr;
    GTAV_REQUIRE(out->w && out->w->grad && (!bias || (out->b && out->b->grad)), "train_enable: the model has no trainable Linear '%s'", n.c_str());
    return 0;
}
static int train_resolve_slots(gtav_dit* h) {
    gtav_dit::Train& t = h->tr;
    t.hs.resize(2 * h->L);
    for (int i = 0; i < 2 * h->L; ++i) {
        char pre[64];
        snprintf(pre, sizeof(pre), "blocks.%d.%c_", i / 2, i % 2 == 0 ? 's' : 't');
        const std::string P_(pre);
        RET_IF(train_linear(h, P_ + "attn.to_qkv", &t.hs[i].qkv, false));
        RET_IF(train_linear(h, P_ + "attn.to_out", &t.hs[i].out));
        RET_IF(train_linear(h, P_ + "mlp.fc1", &t.hs[i].fc1));
        RET_IF(train_linear(h, P_ + "mlp.fc2", &t.hs[i].fc2));
        RET_IF(train_linear(h, P_ + "adaLN_modulation.1", &t.hs[i].ada));
    }
    RET_IF(train_linear(h, "final_layer.linear", &t.fin));
    RET_IF(train_linear(h, "final_layer.adaLN_modulation.1", &t.fin_ada));
    RET_IF(train_linear(h, "x_embedder.proj", &t.pe));
    RET_IF(train_linear(h, "t_embedder.mlp.0", &t.t0));
    RET_IF(train_linear(h, "t_embedder.mlp.2", &t.t2));
    return h->A > 0 ? train_linear(h, "external_cond", &t.ext) : 0;
}

// ... on a LoRA handle (gtav_dit_train_set_lora): the four GEMM Linears of every half-block with their adapter pairs, and the final projection, whose W^T the dX
// chain starts from.  Nothing else is differentiated with respect to its parameters.
static int train_resolve_lora(gtav_dit* h) {
    gtav_dit::Train& t = h->tr;
    t.hs.resize(2 * h->L);
    t.lora.linears.clear();
    static const char* const kLin[4] = {"attn.to_qkv", "attn.to_out", "mlp.fc1", "mlp.fc2"};
    for (int i = 0; i < 2 * h->L; ++i) {
        char pre[64];
        snprintf(pre, sizeof(pre), "blocks.%d.%c_", i / 2, i % 2 == 0 ? 's' : 't');
        gtav_dit::Train::Linear* const lin[4] = {&t.hs[i].qkv, &t.hs[i].out, &t.hs[i].fc1, &t.hs[i].fc2};
        for (int j = 0; j < 4; ++j) {
            const std::string n = std::string(pre) + kLin[j];
            gtav_dit::Train::Linear& l = *lin[j];
            l.w = h->wt.find(n + ".weight"); l.la = h->wt.find(n + ".lora_A.weight"); l.lb = h->wt.find(n + ".lora_B.weight");
            GTAV_REQUIRE(l.w && l.w->master && l.w->wT && l.la && l.la->grad && l.lb && l.lb->grad, "train_enable: the model has no adapted Linear '%s'", n.c_str());
            gtav_dit::Train::Lora::Lin L;
            L.name = n + ".weight"; L.w = l.w; L.a = l.la; L.b = l.lb;
            memset(&L.p, 0, sizeof(L.p));
            L.p.w0 = l.w->master; L.p.a = l.la->master; L.p.b = l.lb->master; L.p.N = l.w->R; L.p.K = l.w->C; L.p.r = t.lora.rank; L.p.s = t.lora.s;
            L.p.w16 = (f16*)l.w->dst; L.p.Cp16 = l.w->Cp; L.p.wT = l.w->wT; L.p.RpT = round_up(l.w->R, 64);
            t.lora.linears.push_back(L);
        }
    }
    t.fin.w = h->wt.find("final_layer.linear.weight");
    GTAV_REQUIRE(t.fin.w && t.fin.w->wT, "train_enable: the model has no final projection");
    return 0;
}
// the device tables of the merge launch (one item per 64 x 64 tile of every adapted weight) and the workspace of the gradient launches
static int train_lora_tables(gtav_dit* h) {
    gtav_dit::Train::Lora& lo = h->tr.lora;
    std::vector<LoraMergeParam> mp;
    std::vector<LoraMergeItem> mi;
    size_t ws = 0;
    for (size_t k = 0; k < lo.linears.size(); ++k) {
        auto& L = lo.linears[k];
        mp.push_back(L.p);
        L.first_item = (int)mi.size();
        L.n_items = (L.p.N / 64) * (L.p.K / 64);
        for (int i = 0; i < L.n_items; ++i) mi.push_back(LoraMergeItem{(int)k, (unsigned)i});
        ws = std::max(ws, lora_grads_workspace_upto(h->Mmax, L.p.N, L.p.K, lo.rank));
    }
    RET_IF(h->arena.alloc_t(&lo.params_dev, mp.size()));
    RET_IF(h->arena.alloc_t(&lo.items_dev, mi.size()));
    GTAV_CHECK_HIP(hipMemcpy(lo.params_dev, mp.data(), mp.size() * sizeof(LoraMergeParam), hipMemcpyHostToDevice));
    GTAV_CHECK_HIP(hipMemcpy(lo.items_dev, mi.data(), mi.size() * sizeof(LoraMergeItem), hipMemcpyHostToDevice));
    lo.n_items = (int)mi.size();
    lo.ws_floats = ws;
    return h->arena.alloc_t(&lo.ws, ws);
}

// every adapted weight's images from its master and its adapters (gtav_dit_finalize, gtav_dit_adamw_step)
int train_lora_merge_all(gtav_dit* h, hipStream_t s) {
    const gtav_dit::Train::Lora& lo = h->tr.lora;
    GTAV_REQUIRE(lo.rank && h->tr.on && lo.n_items, "lora_merge: not a LoRA training handle");
    return operand_ops(h->tr.bf16).lora_merge(lo.params_dev, lo.items_dev, lo.n_items, s);
}
// gtav_dit_set_weight of an adapter or of an adapted base weight: once all three tensors of that Linear have arrived its images are merged again, so the
// order of the uploads does not matter (an upload of the base alone wrote the plain images: WeightTable::set)
// While the averaged weights are swapped in the masters hold the average and the shadow the iterate: the saved activations, the optimizer and every upload belong
// to the other weights.
int train_not_swapped(const gtav_dit* h, const char* who) {
    GTAV_REQUIRE(!h->tr.ema_swapped, "%s: the averaged weights are swapped in (gtav_dit_train_swap_ema); swap the trained weights back first", who);
    return 0;
}
int train_lora_after_set(gtav_dit* h, const std::string& name, hipStream_t s) {
    if (!h->tr.lora.rank || !h->tr.on) return 0;
    for (const auto& L : h->tr.lora.linears) {
        const Slot* sl = h->wt.find(name);
        if (sl != L.w && sl != L.a && sl != L.b) continue;
        if (L.w->set && L.a->set && L.b->set) return operand_ops(h->tr.bf16).lora_merge_one(L.p, 0, s);
        return 0;
    }
    return 0;
}

// gtav_dit_train_enable after its operand-type checks: trainable slots, fp32 masters, AdamW state, saved-activation and backward workspace
static int train_enable_body(gtav_dit* h, float* grad_arena_dev, int64_t grad_arena_numel) {
    for (auto& kv : h->wt.slots) GTAV_REQUIRE(!kv.second.set, "train_enable: call it before any gtav_dit_set_weight (the fp32 masters are filled by set_weight)");
    gtav_dit::Train& t = h->tr;
    Arena& a = h->arena;
    const int D = h->D, L = h->L, Hp = h->Hm_pad;
    const bool lora = t.lora.rank > 0;     // (gtav_dit_train_set_lora): the adapters are the only trainable slots
    GTAV_REQUIRE(!(lora && t.mixed), "train_enable: gtav_dit_train_allow_mixed together with gtav_dit_train_set_lora is not implemented (a type switch remakes the "
                 "2-byte images from the fp32 masters, without the adapters)");
    // Every patch width F = C p^2 the forward takes, but for two refusals.  The patch embedding contracts over Kpe = round_up(F, 64) columns whose pad is zero in
    // both operands (patchify, the weight image), the final projection's gradient dfo is Nf = round_up(F, 64) wide with zero pad columns (mse_bwd_patch).
    const int F = h->C * h->p * h->p, Nf = round_up(h->Nfin, 64);
    GTAV_REQUIRE(h->Hm == h->Hm_pad, "train_enable: a padded MLP width (mlp_ratio * hidden_size = %d, padded to %d) is not implemented for training", h->Hm, h->Hm_pad);
    GTAV_REQUIRE(F % 4 == 0, "train_enable: a patch of in_channels * patch_size^2 = %d features is not implemented for training (the weight-gradient GEMM writes "
                 "multiples of 4 columns)", F);
    GTAV_REQUIRE((size_t)Nf <= (size_t)h->max_rows * D, "train_enable: the final projection's %d features do not fit the bias-gradient scratch (%d x %d)", Nf,
                 h->max_rows, D);
    size_t count = 0;
    std::vector<std::string> names;
    for (auto& kv : h->wt.slots) {
        if (!(lora ? t.lora.trainable_name(kv.first) : WeightTable::trainable_name(kv.first))) continue;
        kv.second.trainable = true;
        t.params.push_back(&kv.second);
        names.push_back(kv.first);
        count += (size_t)kv.second.R * kv.second.C;
    }
    t.grad_count = count;
    if (grad_arena_dev) {
        GTAV_REQUIRE(grad_arena_numel == (int64_t)count, "train_enable: the gradient arena has %lld elements, the model has %lld trainable parameters",
                     (long long)grad_arena_numel, (long long)count);
        t.grad_arena = grad_arena_dev;
    } else {
        RET_IF(a.alloc_t(&t.grad_arena, count));
    }
    size_t off = 0;
    for (size_t pi = 0; pi < t.params.size(); ++pi) {
        Slot* sl = t.params[pi];
        const size_t n = (size_t)sl->R * sl->C;
        sl->grad = t.grad_arena + off;
        off += n;
        RET_IF(a.alloc_t(&sl->am, n));
        RET_IF(a.alloc_t(&sl->av, n));
        if (t.ema_decay > 0.f) RET_IF(a.alloc_t(&sl->ema, n));   // the averaged weights: 4 bytes per trainable parameter more
        if (sl->kind == SLOT_F16_PAD) {
            RET_IF(a.alloc_t(&sl->master, n));
            if (names[pi] != "x_embedder.proj.weight")   // every GEMM weight but the patch embedding needs W^T for dX
                RET_IF(a.alloc_t(&sl->wT, (size_t)round_up(sl->C, 128) * round_up(sl->R, 64)));
        } else {
            sl->master = (float*)sl->dst + sl->c0;
        }
    }
    if (lora) {   // the frozen GEMM weights: the fp32 master the merge starts from (and get_weight returns), W^T for dX; no gradient, no moments
        for (auto& kv : h->wt.slots) {
            Slot& sl = kv.second;
            if (sl.kind != SLOT_F16_PAD) continue;
            RET_IF(a.alloc_t(&sl.master, (size_t)sl.R * sl.C));
            if (kv.first != "x_embedder.proj.weight") RET_IF(a.alloc_t(&sl.wT, (size_t)round_up(sl.C, 128) * round_up(sl.R, 64)));
        }
    }
    RET_IF(a.alloc_t(&t.ctl, 8));
    RET_IF(a.alloc_t(&t.keep, (size_t)h->maxB));
    RET_IF(lora ? train_resolve_lora(h) : train_resolve_slots(h));
    if (lora) RET_IF(train_lora_tables(h));
    t.red_ws_floats = colsum_workspace(h->Mmax > h->max_rows ? h->Mmax : h->max_rows, std::max(std::max(h->Hm_pad, 6 * D), Nf));
    RET_IF(a.alloc_t(&t.red_ws, t.red_ws_floats));
    RET_IF(a.alloc_t(&t.sumsq_part, (size_t)sumsq_parts(count)));
    {
        std::vector<AdamParam> ap;
        std::vector<AdamItem> ai;
        for (size_t pi = 0; pi < t.params.size(); ++pi) {
            Slot* sl = t.params[pi];
            AdamParam d;
            memset(&d, 0, sizeof(d));
            const bool f16w = sl->kind == SLOT_F16_PAD;
            d.p = sl->master; d.ldp = f16w ? sl->C : sl->Cp; d.R = sl->R; d.C = sl->C; d.g = sl->grad; d.m = sl->am; d.v = sl->av; d.e = sl->ema;
            if (f16w) { d.w16 = (f16*)sl->dst; d.Cp16 = sl->Cp; d.wT = sl->wT; d.RpT = round_up(sl->R, 64); }
            ap.push_back(d);
            adam_plan_items(d, (int)pi, ai);   // (a GEMM weight's image sl->dst is never null: w16 set <=> f16w)
        }
        RET_IF(a.alloc_t(&t.adam_params, ap.size()));
        RET_IF(a.alloc_t(&t.adam_items, ai.size()));
        GTAV_CHECK_HIP(hipMemcpy(t.adam_params, ap.data(), ap.size() * sizeof(AdamParam), hipMemcpyHostToDevice));
        GTAV_CHECK_HIP(hipMemcpy(t.adam_items, ai.data(), ai.size() * sizeof(AdamItem), hipMemcpyHostToDevice));
        t.adam_n_items = (int)ai.size();
        t.adam_n[t.bf16 ? 1 : 0] = t.adam_n_items;   // one operand type: one launch over the whole list (gtav_dit_adamw_step)
        if (t.mixed) {
            t.adam_items_host = ai;
            RET_IF(a.alloc_t(&t.range_words, (size_t)h->n_groups));
            h->wt.range_words = t.range_words;   // (a clamped GEMM weight: api_internal.h WeightTable::range_words)
        }
    }
    const size_t Mx = round_up(h->Mmax, 128), Mp = round_up(h->Mmax, 64), Mm = h->Mmax;
    // saved activations (counted: gtav_dit_train_saved_bytes).  Recompute mode: the block inputs r_0, r_4, .. r_4L, three ring states for the ones inside a block,
    // two image sets (spatial / temporal half-block) and one shift per row for every block but the first
    t.saved_bytes = 0;
    auto saved = [&](auto** p, size_t n) -> int {
        RET_IF(a.alloc_t(p, n));
        t.saved_bytes += n * sizeof(**p);
        return 0;
    };
    t.res.assign(4 * L + 1, nullptr);
    if (t.recompute) {
        float* ring[3];
        for (auto& r : ring) RET_IF(saved(&r, Mx * D));
        for (int k = 0; k <= 4 * L; ++k) {
            if (k % 4 == 0) RET_IF(saved(&t.res[k], Mx * D));
            else t.res[k] = ring[k % 4 - 1];
        }
        t.kshift.assign(L, nullptr);
        for (int l = 1; l < L; ++l) RET_IF(saved(&t.kshift[l], Mx));
    } else {
        for (auto& r : t.res) RET_IF(saved(&r, Mx * D));
    }
    t.hb.resize(2 * L);
    for (int i = 0; i < 2 * L; ++i) {
        gtav_dit::Train::HB& b = t.hb[i];
        if (t.recompute && i >= 2) { b = t.hb[i - 2]; continue; }
        RET_IF(saved(&b.xnA, Mx * D)); RET_IF(saved(&b.ao, Mx * D)); RET_IF(saved(&b.y1, Mx * D)); RET_IF(saved(&b.xnB, Mx * D));
        RET_IF(saved(&b.u, Mx * Hp)); RET_IF(saved(&b.hh, Mx * Hp)); RET_IF(saved(&b.y2, Mx * D));
        RET_IF(saved(&b.q, Mx * D));
        if (i % 2 == 0) { RET_IF(saved(&b.k, Mx * D)); RET_IF(saved(&b.v, Mx * D)); }
        else { RET_IF(saved(&b.k, Mx * 2 * D)); b.v = b.k; }
    }
    RET_IF(saved(&t.xnF, Mx * D)); RET_IF(saved(&t.xp, Mx * h->Kpe));
    const size_t R = h->max_rows;
    RET_IF(a.alloc_t(&t.z0, R * D)); RET_IF(a.alloc_t(&t.cpre, R * D));
    RET_IF(a.alloc_t(&t.dres, Mx * D)); RET_IF(a.alloc_t(&t.dtmp, Mx * D)); RET_IF(a.alloc_t(&t.stats, 2 * Mx));
    if (ln_bwd_fused_ok(D)) RET_IF(a.alloc_t(&t.ln_part, ln_bwd_fused_workspace((int)R, h->P, D)));
    RET_IF(a.alloc_t(&t.dmod, R * h->MODW)); RET_IF(a.alloc_t(&t.dSc, R * D)); RET_IF(a.alloc_t(&t.ada_part, ada_bwd_dx_workspace(h->MODW, D, (int)R))); RET_IF(a.alloc_t(&t.dc, R * D)); RET_IF(a.alloc_t(&t.dh0, R * D));
    RET_IF(a.alloc_t(&t.dz0, R * D));
    RET_IF(a.alloc_t(&t.g_d, Mx * D)); RET_IF(a.alloc_t(&t.g_d2, Mx * D)); RET_IF(a.alloc_t(&t.g_h, Mx * Hp)); RET_IF(a.alloc_t(&t.g_u, Mx * Hp)); RET_IF(a.alloc_t(&t.g_qkv, Mx * 3 * D));
    RET_IF(a.alloc_t(&t.dao, Mm * D)); RET_IF(a.alloc_t(&t.dfo, Mx * Nf));
    // (rows of the transposed images, padded to the GEMM's 128-row tiles: dfo^T has Nf rows, xp^T has Kpe)
    // (a LoRA handle runs no dW GEMM: none of the transposed operand buffers)
    const size_t widest = (size_t)std::max(std::max(Hp, 3 * D), std::max(round_up(Nf, 128), round_up(h->Kpe, 128)));
    if (!lora) { RET_IF(a.alloc_t(&t.tA, widest * Mp)); RET_IF(a.alloc_t(&t.tB, widest * Mp)); }
    if (!lora && D % 256 == 0 && Hp % 256 == 0) {   // (rows of the transposed images: fc2 dY / X, fc1, out-proj, QKV)
        const size_t ra[4] = {(size_t)D, (size_t)Hp, (size_t)D, (size_t)3 * D}, rb[4] = {(size_t)Hp, (size_t)D, (size_t)D, (size_t)D};
        for (int i = 0; i < 4; ++i) { RET_IF(a.alloc_t(&t.tAg[i], ra[i] * Mp)); RET_IF(a.alloc_t(&t.tBg[i], rb[i] * Mp)); }
    }
    t.on = true;
    return 0;
}

extern "C" {

// ================================================================================================
// DiT training step: forward with saved activations, backward, AdamW.
// Reference: train_dit.py:649-650 (forward + mse), :680 accelerator.backward, :232-238 AdamW(betas 0.9 / 0.999, eps 1e-7),
// :965-970 clip_grad_norm_ / optimizer.step / zero_grad.  Mixed precision like the reference's bf16 autocast + fp32 master
// weights, with fp16 operands and a loss scale in place of bf16's exponent range: activation gradients travel as fp16 GEMM
// operands multiplied by tr.loss_scale, weight gradients / LayerNorm statistics / the residual-stream gradient are fp32.
// gtav_dit_train_enable_typed(.., GTAV_OPERAND_BF16) runs the same step on bf16 operands (the reference's own autocast type): every launch below that
// reads or writes a 2-byte tensor goes through the operand group's launcher set (h->ops(g): ops_bf16.h OperandOps), the twins of the same kernels.
// ================================================================================================
// Opt-in to training windows of up to max_frames <= 32 frames (the default, 8, is what train_window_ok otherwise enforces): between create and train_enable only.
int gtav_dit_train_allow_window(gtav_dit* h, int32_t max_frames) {
    GTAV_REQUIRE(h, "train_allow_window: null handle");
    GTAV_REQUIRE(!h->tr.on, "train_allow_window: training is already enabled on this handle (call it between gtav_dit_create and gtav_dit_train_enable)");
    GTAV_REQUIRE(max_frames >= 8 && max_frames <= 32, "train_allow_window: max_frames=%d outside [8, 32]", max_frames);
    h->tr.window = max_frames;
    return 0;
}

// Opt-in to activation recomputation (api_internal.h Train::recompute): between create and train_enable only, like gtav_dit_train_allow_window.
int gtav_dit_train_set_recompute(gtav_dit* h, int32_t enable) {
    GTAV_REQUIRE(h, "train_set_recompute: null handle");
    GTAV_REQUIRE(!h->tr.on, "train_set_recompute: training is already enabled on this handle (call it between gtav_dit_create and gtav_dit_train_enable)");
    h->tr.recompute = enable != 0;
    return 0;
}

// Opt-in to operand groups of both types on one training handle (api_internal.h Train::mixed): between create and train_enable only, like the two above.
int gtav_dit_train_allow_mixed(gtav_dit* h, int32_t enable) {
    GTAV_REQUIRE(h, "train_allow_mixed: null handle");
    GTAV_REQUIRE(!h->tr.on, "train_allow_mixed: training is already enabled on this handle (call it between gtav_dit_create and gtav_dit_train_enable)");
    GTAV_REQUIRE(!(enable && h->tr.lora.rank), "train_allow_mixed: mixed operand groups together with low-rank adapters (gtav_dit_train_set_lora) are not implemented");
    h->tr.mixed = enable != 0;
    return 0;
}

// Opt-in to low-rank adapter training (api_internal.h Train::Lora; DESIGN.md 7 "Low-rank adapters"): between create and train_enable only, like the three above.
// Adds the adapter pairs of the four GEMM Linears of every half-block to the weight table as fp32 slots.
int gtav_dit_train_set_lora(gtav_dit* h, int32_t rank, float alpha) {
    GTAV_REQUIRE(h, "train_set_lora: null handle");
    GTAV_REQUIRE(!h->tr.on, "train_set_lora: training is already enabled on this handle (call it between gtav_dit_create and gtav_dit_train_enable)");
    GTAV_REQUIRE(lora_rank_ok(rank), "train_set_lora: rank %d (the adapters fill whole MFMA tiles: 16, 32 or 64)", rank);
    GTAV_REQUIRE(alpha > 0.f && std::isfinite(alpha), "train_set_lora: alpha=%g must be a positive number", (double)alpha);
    GTAV_REQUIRE(!h->tr.mixed, "train_set_lora: low-rank adapters together with mixed operand groups (gtav_dit_train_allow_mixed) are not implemented");
    GTAV_REQUIRE(h->tr.lora.rank == 0, "train_set_lora: the adapters of this handle exist already (rank %d)", h->tr.lora.rank);
    GTAV_REQUIRE(h->D % 64 == 0 && h->Hm % 64 == 0 && h->Hm == h->Hm_pad, "train_set_lora: hidden_size=%d and the MLP width %d must be multiples of 64 (the merge works "
                 "on 64 x 64 tiles)", h->D, h->Hm);
    static const char* const kLin[4] = {"attn.to_qkv", "attn.to_out", "mlp.fc1", "mlp.fc2"};
    const int D = h->D, NK[4][2] = {{3 * D, D}, {D, D}, {h->Hm, D}, {D, h->Hm}};
    for (int i = 0; i < 2 * h->L; ++i)
        for (int j = 0; j < 4; ++j) {
            char pre[96];
            snprintf(pre, sizeof(pre), "blocks.%d.%c_%s", i / 2, i % 2 == 0 ? 's' : 't', kLin[j]);
            float *pa = nullptr, *pb = nullptr;
            RET_IF(h->arena.alloc_t(&pa, (size_t)rank * NK[j][1]));
            RET_IF(h->arena.alloc_t(&pb, (size_t)NK[j][0] * rank));
            h->wt.add_f32(std::string(pre) + ".lora_A.weight", rank, NK[j][1], pa, NK[j][1]);
            h->wt.add_f32(std::string(pre) + ".lora_B.weight", NK[j][0], rank, pb, rank);
        }
    h->tr.lora.rank = rank; h->tr.lora.alpha = alpha; h->tr.lora.s = alpha / (float)rank;
    h->finalized = false;
    return 0;
}

// Opt-in to averaged weights (api_internal.h Train::ema_decay; DESIGN.md 7 "Averaged weights").  Between create and train_enable it turns the shadow on (allocated
// by train_enable); on an enabled handle that has one it changes the decay and the warm-up of the steps to come.  The decay is checked first: a bad one is refused
// whatever the handle.
int gtav_dit_train_set_ema(gtav_dit* h, float decay, int32_t warmup) {
    GTAV_REQUIRE(decay > 0.f && decay < 1.f, "train_set_ema: decay=%g outside (0, 1)", (double)decay);
    GTAV_REQUIRE(h, "train_set_ema: null handle");
    GTAV_REQUIRE(!h->tr.on || h->tr.ema_decay > 0.f, "train_set_ema: training is already enabled on this handle without averaged weights; the shadow is allocated by "
                 "gtav_dit_train_enable and cannot be turned on or off afterwards (call it between gtav_dit_create and gtav_dit_train_enable)");
    h->tr.ema_decay = decay;
    h->tr.ema_warmup = warmup != 0;
    return 0;
}

// fp32 W0 + s B A of one adapted weight, torch layout: what the merge launch casts into the images (the same device function)
int gtav_dit_lora_get_merged(gtav_dit* h, const char* name, float* dst, int64_t numel, void* stream) {
    GTAV_REQUIRE(h && name && dst, "lora_get_merged: null argument");
    GTAV_REQUIRE(h->tr.lora.rank && h->tr.on, "lora_get_merged: not a LoRA training handle (gtav_dit_train_set_lora, gtav_dit_train_enable)");
    for (const auto& L : h->tr.lora.linears) {
        if (L.name != name) continue;
        GTAV_REQUIRE(numel == (int64_t)L.p.N * L.p.K, "lora_get_merged: '%s' has %d x %d elements, got %lld", name, L.p.N, L.p.K, (long long)numel);
        GTAV_REQUIRE(L.w->set && L.a->set && L.b->set, "lora_get_merged: '%s' or its adapters were not set", name);
        LoraMergeParam P = L.p;
        P.w32 = dst;
        return operand_ops(h->tr.bf16).lora_merge_one(P, 1, (hipStream_t)stream);
    }
    GTAV_REQUIRE(false, "lora_get_merged: '%s' is not an adapted weight (the to_qkv, to_out, fc1 and fc2 weights of the blocks are)", name);
    return 0;
}

int gtav_dit_train_saved_bytes(gtav_dit* h, int64_t* bytes) {
    GTAV_REQUIRE(h && bytes, "train_saved_bytes: null argument");
    GTAV_REQUIRE(h->tr.on, "train_saved_bytes: training is not enabled");
    *bytes = (int64_t)h->tr.saved_bytes;
    return 0;
}

int gtav_dit_train_enable(gtav_dit* h, float* grad_arena_dev, int64_t grad_arena_numel) {
    GTAV_REQUIRE(h, "train_enable: null handle");
    RET_IF(train_window_ok(h));
    GTAV_REQUIRE(!h->tr.on, "train_enable: already enabled");
    GTAV_REQUIRE(!h->any_bf16, "train_enable: the training step runs on fp16 operands (gtav_dit_set_operand_dtype(h, -1, GTAV_OPERAND_F16) first)");
    return train_enable_body(h, grad_arena_dev, grad_arena_numel);
}

int gtav_dit_train_enable_typed(gtav_dit* h, float* grad_arena_dev, int64_t grad_arena_numel, int32_t dtype) {
    GTAV_REQUIRE(h, "train_enable_typed: null handle");
    GTAV_REQUIRE(dtype == GTAV_OPERAND_F16 || dtype == GTAV_OPERAND_BF16, "train_enable_typed: dtype %d (0 = fp16, 1 = bf16)", dtype);
    if (dtype == GTAV_OPERAND_F16) return gtav_dit_train_enable(h, grad_arena_dev, grad_arena_numel);
    RET_IF(train_window_ok(h));   // before the type switch below changes the handle
    GTAV_REQUIRE(!h->tr.on, "train_enable: already enabled");
    int nb = 0;
    for (unsigned char b : h->grp_bf16) nb += b != 0;
    GTAV_REQUIRE(nb == 0 || nb == h->n_groups, "train_enable_typed: %d of the %d operand groups are bf16; a training handle has one operand type for every group", nb,
                 h->n_groups);
    // (before the type switch, which un-sets the weight slots it converts)
    for (auto& kv : h->wt.slots) GTAV_REQUIRE(!kv.second.set, "train_enable: call it before any gtav_dit_set_weight (the fp32 masters are filled by set_weight)");
    RET_IF(gtav_dit_set_operand_dtype(h, -1, GTAV_OPERAND_BF16));
    h->tr.bf16 = true;
    h->tr.loss_scale = 1.0f;   // bf16 has fp32's exponent range: the reference trains it without a scaler (gtav_dit_set_loss_scale still applies)
    return train_enable_body(h, grad_arena_dev, grad_arena_numel);
}

}  // extern "C"

// Where a launch of the training forward raises its saturation bits: on a mixed-capable handle (gtav_dit_train_allow_mixed) in its operand group's word, which
// launch_err_fold moves into word 0 and the group's sticky word; on every other handle in word 0, as ever.
static int* train_fwd_err(const gtav_dit* h, int g) { return h->tr.mixed ? h->err_of(g) : h->err_flag; }

// The one 2-byte tensor that crosses a group boundary: the branch image y2 of a half-block's fc2 (LnPending::y_save) is written by the LayerNorm launch that
// applies the pending update, which belongs to the NEXT group (the next half-block's, or the final layer's), and read by the producer's gate backward on the
// producer's launcher set.  Where the two groups differ in type the producer's set writes it here, with the LayerNorm kernel's sum, and the LayerNorm keeps none.
static int train_branch_seam(gtav_dit* h, int producer, int consumer, DeferredResid& rd, hipStream_t s) {
    if (!rd.pending || !rd.pend.y_save || h->grp_bf16[producer] == h->grp_bf16[consumer]) return 0;
    RET_IF(h->ops(producer).branch_rows(rd.pend.parts, rd.pend.nsplit, rd.pend.slab_stride, rd.pend.ld, rd.pend.bias, rd.pend.y_save, rd.M, rd.N,
                                        train_fwd_err(h, producer), s));
    rd.pend.y_save = nullptr;
    return 0;
}

// Both half-blocks of block l of the training forward (gtav_dit_train_forward runs it for l = 0 .. L - 1).  Every residual GEMM stores split-K slabs and leaves
// the update to the next LayerNorm launch (`rd`): on return the block's last fc2 branch is still pending, and the first LayerNorm of block l + 1 (or the final
// layer's) applies it, writes r_{4l+4} and the branch image y2.
// rerun (recompute mode, train_rerun_block): the block starts from its stored input r_4l, which already holds the update that the forward's first LayerNorm
// applied, so that launch runs without one — on the row-block kernel and with the statistics' shift the forward's launch kept (LnPending::k_load).
static int train_block_forward(gtav_dit* h, int l, int B, int T, bool rerun, DeferredResid& rd, hipStream_t s) {
    gtav_dit::Train& tr = h->tr;
    const int D = h->D, P = h->P, NB = B * T, M = NB * P;
    for (int hf = 0; hf < 2; ++hf) {
        const int i = l * 2 + hf;
        const gtav_dit::Half& w = h->halves[i];
        gtav_dit::Train::HB& b = tr.hb[i];
        const float* mb = h->mod + (size_t)i * 6 * D;
        const OperandOps& o = h->ops(i);
        int* const ef = train_fwd_err(h, i);
        auto gate = [&](const float* g) { return ResidGate{g, h->MODW, nullptr, P}; };
        // LN1 normalises r_{2i} (= r_{2i-1} + gate (fc2 of the previous half-block), written to res[2i] by this launch)
        const bool from_stored = rerun && hf == 0 && l > 0;
        if (from_stored) RET_IF(rd.load_shift(tr.kshift[l]));
        else if (tr.recompute && hf == 0 && l > 0) rd.save_shift(tr.kshift[l]);   // (l > 0: the previous block's fc2 is pending)
        if (i > 0 && !from_stored) RET_IF(train_branch_seam(h, i - 1, i, rd, s));
        RET_IF(o.ln_modulate(from_stored ? tr.res[2 * i] : i == 0 ? tr.res[0] : tr.res[2 * i - 1], D, b.xnA, D, M, D, mb, mb + D, h->MODW, nullptr, P, rd.take(), ef, s));
        GemmParams g = gemm_params(b.xnA, D, w.w_qkv, M, 3 * D, D);
        g.D = D; g.S = P; g.err_flag = ef;
        if (hf == 0) { g.qkv_mode = QKV_SPATIAL; g.q = b.q; g.k = b.k; g.v = b.v; g.rope_cs = h->rope_s.cs_dev; }
        else { g.qkv_mode = QKV_TEMPORAL; g.q = b.q; g.k = b.k; g.v = b.k; g.Tq = T; g.t0 = 0; g.Tmax = h->maxT; g.rope_cs = h->rope_t.cs_dev; }
        RET_IF(o.gemm(g, EPI_QKV, s));
        if (hf == 0) RET_IF(o.attn_spatial(b.q, b.k, b.v, b.ao, NB, h->heads, P, s, false));
        else RET_IF(o.attn_temporal(b.q, b.k, b.ao, B, P, D, T, 0, h->maxT, s));
        RET_IF(rd.gemm(o, PC_OUT, b.ao, D, w.w_out, D, w.b_out, gate(mb + 2 * D), false, kNoPrefetch, tr.res[2 * i + 1], b.y1));
        RET_IF(o.ln_modulate(tr.res[2 * i], D, b.xnB, D, M, D, mb + 3 * D, mb + 4 * D, h->MODW, nullptr, P, rd.take(), ef, s));
        GemmParams fc1 = gemm_params(b.xnB, D, w.w_fc1, M, h->Hm, D);
        fc1.bias = w.b_fc1; fc1.out = b.u; fc1.ldo = h->Hm_pad; fc1.err_flag = ef;
        if (g_fuse_gelu_fwd) fc1.out2 = b.hh;             // h = GELU(u) as a second image of the same epilogue (gemm.h out2)
        RET_IF(o.gemm(fc1, EPI_F16_TILED, s));            // the pre-activation is kept: gelu'(u) in the backward pass
        if (!g_fuse_gelu_fwd) RET_IF(h->ops(i).gelu_tiled(b.u, b.hh, (size_t)round_up(M, 128) * h->Hm_pad, s));
        RET_IF(rd.gemm(o, PC_FC2, b.hh, h->Hm_pad, w.w_fc2, h->Hm_pad, w.b_fc2, gate(mb + 5 * D), false, kNoPrefetch, tr.res[2 * i + 2], b.y2));
    }
    return 0;
}

// Recompute mode: the forward of block l of the last gtav_dit_train_forward again, from its stored input state into the ring states and the two image sets: the
// same launches on the same inputs, so the same bits (the first LayerNorm: see train_block_forward).  The block's last fc2 branch was applied, and its image y2
// written, by the first LayerNorm of block l + 1: that launch runs again at the end (it rewrites r_{4l+4} and kshift[l + 1] with the values they hold; its
// normalised output is not needed and goes to the backward workspace g_d, free between two blocks' backward passes).  The last block's activations are in
// place after the forward; a second backward pass over the same forward re-runs it too, and ends with the final layer's LayerNorm as the forward does.
static int train_rerun_block(gtav_dit* h, int l, hipStream_t s) {
    gtav_dit::Train& tr = h->tr;
    const int D = h->D, L = h->L, i = 2 * l + 2;
    GTAV_REQUIRE(l >= 0 && l < L, "train_backward: no block %d to re-run", l);
    DeferredResid rd{h->parts, h->parts_rows * (size_t)D, nullptr, tr.M, D, nullptr, s};
    tr.rc_block = -1;
    RET_IF(train_block_forward(h, l, tr.B, tr.T, true, rd, s));
    const float* mb = h->mod + (size_t)i * 6 * D;   // (i = 2 L: the final layer's shift and scale)
    const bool last = l == L - 1;   // (then 2 i - 1 = 4 L - 1, and the launch is the final layer's)
    if (!last) rd.save_shift(tr.kshift[l + 1]);
    const int gn = last ? 2 * L + 1 : i;   // the group of that launch
    RET_IF(train_branch_seam(h, i - 1, gn, rd, s));
    RET_IF(h->ops(gn).ln_modulate(tr.res[2 * i - 1], D, last ? tr.xnF : tr.g_d, D, tr.M, D, mb, mb + D, h->MODW, nullptr, h->P, rd.take(), train_fwd_err(h, gn), s));
    tr.rc_block = l;
    return 0;
}

extern "C" {


int gtav_dit_train_param_count(gtav_dit* h, int64_t* numel) {
    GTAV_REQUIRE(h && numel, "train_param_count: null argument");
    int64_t c = 0;
    for (auto& kv : h->wt.slots)
        if (h->tr.lora.rank ? h->tr.lora.trainable_name(kv.first) : WeightTable::trainable_name(kv.first)) c += (int64_t)kv.second.R * kv.second.C;
    *numel = c;
    return 0;
}

int gtav_dit_set_loss_scale(gtav_dit* h, float scale) {
    GTAV_REQUIRE(h && scale > 0.f, "set_loss_scale: bad argument");
    h->tr.loss_scale = scale;
    return 0;
}

int gtav_dit_set_grad_divisor(gtav_dit* h, float divisor) {
    GTAV_REQUIRE(h && h->tr.on && divisor >= 1.0f, "set_grad_divisor: bad argument");
    h->tr.grad_div = divisor;
    return 0;
}
int gtav_dit_zero_grad(gtav_dit* h, void* stream) {
    GTAV_REQUIRE(h && h->tr.on, "zero_grad: training is not enabled");
    // (hipMemsetAsync splits 2.4 GB into ~600 fill launches of 4 MB: 3.8 ms per step in the rocprofv3 trace; one grid-stride kernel: 0.5 ms)
    RET_IF(launch_fill_f32(h->tr.grad_arena, h->tr.grad_count, 0.f, (hipStream_t)stream));
    // a training step starts here: saturation / non-finite bits raised by an earlier forward on this handle (validation, predict) are not this step's
    // overflow — clear them so that only the step's own stores can make the optimizer skip (gtav_dit_check reports inference saturation before that)
    // (a mixed-capable handle's training forward raises its bits in the group words, where an inference forward raises its own: those are set aside in word 1
    // — neither a skip nor a type switch, and still reported by gtav_dit_check; the sticky words are not touched)
    if (h->tr.mixed) RET_IF(launch_err_fold(h->err_flag, nullptr, 1, h->n_groups, (hipStream_t)stream));
    return launch_err_clear(h->err_flag, ERR_F16_SAT | ERR_NONFINITE, (hipStream_t)stream);
}

// raw (loss-scaled) gradient of one parameter, torch layout; the caller divides by the loss scale
int gtav_dit_get_grad(gtav_dit* h, const char* name, float* dst, int64_t numel, void* stream) {
    GTAV_REQUIRE(h && name && dst && h->tr.on, "get_grad: bad argument / training is not enabled");
    auto it = h->wt.slots.find(name);
    GTAV_REQUIRE(it != h->wt.slots.end() && it->second.grad, "get_grad: '%s' is not a trainable parameter", name);
    GTAV_REQUIRE(numel == (int64_t)it->second.R * it->second.C, "get_grad: '%s' size mismatch", name);
    GTAV_CHECK_HIP(hipMemcpyAsync(dst, it->second.grad, numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

static int train_forward_impl(gtav_dit* h, const float* x, const int64_t* t64, const float* actions, const int32_t* keep, float* out, int32_t B, int32_t T, void* stream);

int gtav_dit_train_forward(gtav_dit* h, const float* x, const int64_t* t64, const float* actions, float* out, int32_t B, int32_t T, void* stream) {
    return train_forward_impl(h, x, t64, actions, nullptr, out, B, T, stream);
}

int gtav_dit_train_forward_keep(gtav_dit* h, const float* x, const int64_t* t64, const float* actions, const int32_t* keep, float* out, int32_t B, int32_t T,
                                void* stream) {
    GTAV_REQUIRE(!keep || actions, "train_forward_keep: a keep mask without actions (there is nothing to drop)");
    return train_forward_impl(h, x, t64, actions, keep, out, B, T, stream);
}

}  // extern "C"

// keep (device, B flags, optional): sample b with keep[b] == 0 is conditioned as external_cond=None for all its frames (gtav_dit_train_forward_keep)
static int train_forward_impl(gtav_dit* h, const float* x, const int64_t* t64, const float* actions, const int32_t* keep, float* out, int32_t B, int32_t T, void* stream) {
    GTAV_REQUIRE(h && x && t64 && out, "train_forward: null argument");
    GTAV_REQUIRE(h->tr.on && h->finalized, "train_forward: call gtav_dit_train_enable, load the weights and finalize first");
    RET_IF(train_not_swapped(h, "train_forward"));
    GTAV_REQUIRE(B >= 1 && B <= h->maxB && T >= 1 && T <= h->maxT, "train_forward: B=%d T=%d outside capacity (%d, %d)", B, T, h->maxB, h->maxT);
    GTAV_REQUIRE(!actions || h->A > 0, "train_forward: model has no external_cond");
    hipStream_t s = (hipStream_t)stream;
    gtav_dit::Train& tr = h->tr;
    const int D = h->D, P = h->P, NB = B * T, M = NB * P, L = h->L, rows = NB, ldhc = D + h->Apad;
    h->prepared.valid = false;
    h->kvrec.valid = false;
    tr.rc_block = -1;   // (recompute mode: this forward overwrites the ring states and the image sets; if it fails partway, no block is in place)
    // conditioning path with its pre-activations kept (dit_cond applies SiLU inside the skinny GEMM)
    RET_IF(launch_cond_inputs(t64, rows, 1, nullptr, 0, h->sincos, h->E, actions, h->A, 0, rows, h->A, h->HC, ldhc, D, h->Apad, h->err_flag, s));
    RET_IF(launch_skinny_f32(h->E, 256, h->w_t0, h->b_t0, tr.z0, D, rows, D, 256, 0, s));
    RET_IF(launch_silu(tr.z0, D, h->HC, ldhc, rows, D, s));
    if (keep) {
        // per-sample action dropout: a dropped sample's rows lose their action columns, and every row gets ITS bias — b_t2a (kept) or b_t2 (dropped) — by the one
        // fp32 add the GEMM epilogue would have made: all ones is the plain forward with actions bit for bit, all zeros the forward with actions = NULL
        GTAV_CHECK_HIP(hipMemcpyAsync(tr.keep, keep, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        RET_IF(launch_keep_mask_cols(h->HC + D, ldhc, rows, h->Apad, T, tr.keep, s));
        RET_IF(launch_skinny_f32(h->HC, ldhc, h->w_t2cat, nullptr, tr.cpre, D, rows, D, ldhc, 0, s));
        RET_IF(launch_keep_add_bias(tr.cpre, D, rows, D, T, tr.keep, h->b_t2a, h->b_t2, s));
    } else {
        RET_IF(launch_skinny_f32(h->HC, ldhc, h->w_t2cat, actions ? h->b_t2a : h->b_t2, tr.cpre, D, rows, D, ldhc, 0, s));
    }
    RET_IF(launch_silu(tr.cpre, D, h->Sc, D, rows, D, s));
    RET_IF(launch_skinny_f32(h->Sc, D, h->w_ada, h->b_ada, h->mod, h->MODW, rows, h->MODW, D, 0, s));
    const float* mod = h->mod;
    const OperandOps& oe = h->ops(2 * L), &ofin = h->ops(2 * L + 1);   // patch embedding, final layer (the half-blocks: h->ops(i) below)
    RET_IF(oe.patchify(x, nullptr, NB, h->C, h->H, h->W, h->p, tr.xp, h->Kpe, 1.f, 0.f, train_fwd_err(h, 2 * L), s));
    GemmParams g = gemm_params(tr.xp, h->Kpe, h->w_pe, M, D, h->Kpe);
    g.bias = h->b_pe; g.out = tr.res[0]; g.ldo = D;
    RET_IF(oe.gemm(g, EPI_F32, s));
    DeferredResid rd{h->parts, h->parts_rows * (size_t)D, nullptr, M, D, nullptr, s};   // no in-place target (the backward pass needs every state and branch), no profiler
    for (int l = 0; l < L; ++l) RET_IF(train_block_forward(h, l, B, T, false, rd, s));
    const float* mf = mod + (size_t)L * 12 * D;
    RET_IF(train_branch_seam(h, 2 * L - 1, 2 * L + 1, rd, s));
    RET_IF(ofin.ln_modulate(tr.res[4 * L - 1], D, tr.xnF, D, M, D, mf, mf + D, h->MODW, nullptr, P, rd.take(), train_fwd_err(h, 2 * L + 1), s));
    g = gemm_params(tr.xnF, D, h->w_final, M, h->Nfin, D);
    g.bias = h->b_final; g.out = h->fo; g.ldo = h->Nfin;
    RET_IF(ofin.gemm(g, EPI_F32, s));
    RET_IF(launch_unpatchify(h->fo, h->Nfin, out, NB, h->C, h->H, h->W, h->p, 0, 1.f, 0.f, s));
    // (mixed-capable handles) the groups' bits of this forward into word 0, where the backward's publish and the optimizer look, and into the sticky words
    if (tr.mixed) RET_IF(launch_err_fold(h->err_flag, tr.range_words, 0, h->n_groups, s));
    tr.B = B; tr.T = T; tr.M = M; tr.Mp = round_up(M, 64); tr.rows = rows; tr.have_actions = actions != nullptr; tr.have_fwd = true;
    tr.have_keep = keep != nullptr;
    tr.rc_block = L - 1;   // (recompute mode: the ring states and the two image sets hold the last block)
    return 0;
}

extern "C" {

// Residual stream of the last training forward after k branch additions (every block adds four branches: spatial attention, spatial
// MLP, temporal attention, temporal MLP): k = 0 is the patch embedding output, k = 4 (l + 1) the output of block l, k = 4 L the input of
// the final layer.  fp32 [B T P][D] in token order (b, t, p): per-block parity taps (model/dit.py:370-372).
int gtav_dit_train_get_residual(gtav_dit* h, int32_t k, float* dst, int64_t numel, void* stream) {
    GTAV_REQUIRE(h && dst && h->tr.on && h->tr.have_fwd, "train_get_residual: no saved forward");
    GTAV_REQUIRE(k >= 0 && k <= 4 * h->L, "train_get_residual: k=%d must be in [0, %d]", k, 4 * h->L);
    GTAV_REQUIRE(!h->tr.recompute || k % 4 == 0, "train_get_residual: k=%d is a state inside a block, which a handle in recompute mode (gtav_dit_train_set_recompute) "
                 "does not keep: k must be a multiple of 4 (block inputs, 4 * depth = the input of the final layer)", k);
    GTAV_REQUIRE(numel == (int64_t)h->tr.M * h->D, "train_get_residual: expected %lld elements", (long long)h->tr.M * h->D);
    GTAV_CHECK_HIP(hipMemcpyAsync(dst, h->tr.res[k], numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

}  // extern "C"

// One call of the backward pass: what its parts share (set up by gtav_dit_train_backward_phases from the shapes of the saved forward), and the parts
struct TrainBackward {
    gtav_dit* h;
    gtav_dit::Train& tr;
    hipStream_t s;
    const int D, P, L, B, T, M, Mp, NB, rows, Hp, MODW;
    const OperandOps* op;   // launcher set of the operand group being differentiated (final layer, half-block i, patch embedding): set where each part begins
    bool defer_dw = false, tn_dw, fuse_ln, fuse_gate, defer_bias;   // which fusions the shapes of this step allow (the constructor says when)
    const bool lora;        // a LoRA handle (Train::Lora): adapter gradients in place of dW, no bias / adaLN / final-layer / embedder parameter gradients
    GemmDwGroup dwg[GEMM_DW_MAX_GROUPS];   // the pending grouped weight gradients
    int ndw = 0;

    TrainBackward(gtav_dit* h_, hipStream_t s_)
        : h(h_), tr(h_->tr), s(s_), D(h->D), P(h->P), L(h->L), B(tr.B), T(tr.T), M(tr.M), Mp(tr.Mp), NB(B * T), rows(tr.rows), Hp(h->Hm_pad), MODW(h->MODW), op(&h->ops(2 * L + 1)), lora(h_->tr.lora.rank > 0) {
        // Half-blocks of production widths defer their four dW GEMMs into ONE grouped launch of 256 x 256 tiles (flush_dw; gemm.h)
        if (tr.tAg[0] && g_dw_grouped) {
            const GemmDwGroup probe[4] = {{tr.tAg[0], tr.tBg[0], tr.dres, D, Hp, Hp}, {tr.tAg[1], tr.tBg[1], tr.dres, Hp, D, D}, {tr.tAg[2], tr.tBg[2], tr.dres, D, D, D},
                                          {tr.tAg[3], tr.tBg[3], tr.dres, 3 * D, D, D}};
            defer_dw = gemm_dw_grouped_ok(probe, 4, Mp);
        }
        // Whole 128-token row tiles: the grouped launch contracts over the rows of the tile-major operands THEMSELVES (transposing LDS reads, gemm.hip
        // mainloop256_tn) — no transposed copies (8 of the 17 us transposes per half-block).  The operands must then live until flush_dw: the out-projection's
        // dY gets a buffer of its own (g_d2), the saved activations and g_u / g_qkv are not rewritten inside a half-block.
        tn_dw = defer_dw && g_dw_tn && M % 128 == 0;
        fuse_ln = g_fuse_ln && tr.ln_part && M == NB * P && NB <= rows;   // LayerNorm backward and its per-frame reduction in one launch (train.hip ln_mod_bwd_fused_kernel)
        // gate backward, the gate's own gradient and the bias gradient of the Linear in front of it in one pass over dres (train.hip gate_bwd_fused_kernel): the
        // per-frame partial sums of the bias gradient (NB x D floats) must fit the reduction workspace
        fuse_gate = g_fuse_gate && M == NB * P && (size_t)NB * D <= tr.red_ws_floats;
        // ... and the partial sums of the half-block's three bias gradients go to three regions of the workspace, which ONE launch adds at the end of the half-block
        defer_bias = fuse_gate && g_fuse_gelu && (size_t)2 * NB * D + (size_t)gelu_bwd_colsum_splits(M) * Hp <= tr.red_ws_floats;
    }
    // dX = dY W: A = dY tile-major [M][Kc], WT = tile-major W^T [N][Kc]
    int gemm_dx(const f16* A, const f16* WT, int N, int Kc, int epi, void* out, int ldo) {
        GemmParams q = gemm_params(A, Kc, WT, M, N, Kc);
        q.out = out; q.ldo = ldo; q.err_flag = h->err_flag;
        return op->gemm(q, epi, s);
    }
    int flush_dw() {
        if (!ndw) return 0;
        const int n = ndw;
        ndw = 0;
        return op->gemm_dw_grouped(dwg, n, tn_dw ? M : Mp, h->err_flag, s, tn_dw);
    }
    // dW[n][k] += sum_m dY[m][n] X[m][k]: both operands transposed to [.][Mp] (tokens are the contraction), accumulating epilogue; slot_i >= 0: one of the four of a
    // half-block (fc2, fc1, out-proj, QKV), deferred into its grouped launch where that is on
    // Kv < K (the patch embedding at C p^2 % 64 != 0): X carries K - Kv zero pad columns which the gradient, contiguous [N][Kv], has no room for: the
    // transposed-operand GEMM writes the first Kv of its K features with ldo = Kv (the other forms write whole 128 / 256-column tiles)
    int gemm_dw(const f16* dY, int N, const f16* X, int K, float* grad, int slot_i = -1, int Kv = 0) {
        GTAV_REQUIRE(!lora, "train_backward: a LoRA handle computes no full weight gradient");
        if (Kv > 0 && Kv < K) {
            RET_IF(op->transpose_tiled(dY, M, N, tr.tA, s));
            RET_IF(op->transpose_tiled(X, M, K, tr.tB, s));
            GemmParams q = gemm_params(tr.tA, Mp, tr.tB, N, Kv, Mp);
            q.out = grad; q.ldo = Kv;
            return op->gemm(q, EPI_RESID, s);
        }
        if (tn_dw && slot_i >= 0) {
            dwg[ndw++] = GemmDwGroup{dY, X, grad, N, K, K};
            return 0;
        }
        if (defer_dw && slot_i >= 0) {
            RET_IF(op->transpose_tiled(dY, M, N, tr.tAg[slot_i], s));
            RET_IF(op->transpose_tiled(X, M, K, tr.tBg[slot_i], s));
            dwg[ndw++] = GemmDwGroup{tr.tAg[slot_i], tr.tBg[slot_i], grad, N, K, K};
            return 0;
        }
        if (gemm_tn_pays(N, K, M)) {   // contraction over the rows of the tile-major operands themselves (transposing LDS reads): no transposes
            GemmParams q = gemm_params(dY, N, X, N, K, M);
            q.out = grad; q.ldo = K;
            return op->gemm_tn(q, s);
        }
        RET_IF(op->transpose_tiled(dY, M, N, tr.tA, s));
        RET_IF(op->transpose_tiled(X, M, K, tr.tB, s));
        GemmParams q = gemm_params(tr.tA, Mp, tr.tB, N, K, Mp);
        q.out = grad; q.ldo = K;
        return op->gemm(q, EPI_RESID, s);
    }
    // the weight gradient of one of a half-block's four Linears: the full dW, or on a LoRA handle the gradients of its adapter pair (train.hip launch_lora_grads:
    // three launches at once, nothing deferred, so dY and X need not outlive the call)
    int linear_dw(const gtav_dit::Train::Linear& l, const f16* dY, int N, const f16* X, int K, int slot_i) {
        if (!lora) return gemm_dw(dY, N, X, K, l.w->grad, slot_i);
        return op->lora_grads(X, dY, l.la->master, l.lb->master, M, N, K, tr.lora.rank, tr.lora.s, l.la->grad, l.lb->grad, tr.lora.ws, tr.lora.ws_floats, h->err_flag, s);
    }
    static float* bias_grad(const gtav_dit::Train::Linear& l) { return l.b ? l.b->grad : nullptr; }   // (null on a LoRA handle: the biases are frozen)
    int ln_bwd(const float* dxn, const float* x, const float* scale, int accumulate, float* dshift, float* dscale) {
        if (fuse_ln) return launch_ln_mod_bwd_fused(dxn, x, scale, MODW, NB, P, D, tr.dres, accumulate, dshift, dscale, tr.ln_part, s);
        RET_IF(launch_ln_mod_bwd(dxn, x, scale, MODW, P, M, D, tr.dres, accumulate, tr.stats, s));
        return launch_frame_reduce_ln(dxn, x, tr.stats, NB, P, D, dshift, dscale, MODW, s);
    }
    // gradient of one adaLN projection (rows [row0, row0 + n) of W_ada / b_ada) from the dmod columns its LayerNorm / gate backward filled
    int ada_grads(size_t row0, int n, const Slot* w, const Slot* b) {
        RET_IF(launch_gemm_tn_f32(tr.dmod + row0, MODW, h->Sc, D, rows, n, D, w->grad, D, s));
        return launch_colsum_f32(tr.dmod + row0, MODW, rows, n, b->grad, tr.red_ws, s);
    }
    // r' = r + gate y backward: dY of the branch (tr.dres gate -> g_out), the gate's gradient (dgate), and the bias gradient of the Linear that made y (ws: its
    // partial sums under fuse_gate; deferred: left there for the one launch at the end of the half-block)
    int gate_bwd(const f16* y, const float* gate, float* dgate, f16* g_out, float* dbias, float* ws) {
        if (fuse_gate) return op->gate_bwd_fused(tr.dres, y, gate, MODW, NB, P, D, g_out, dgate, defer_bias ? nullptr : dbias, ws, h->err_flag, s);
        RET_IF(op->gate_bwd(tr.dres, gate, MODW, P, M, D, g_out, h->err_flag, s));
        RET_IF(op->frame_reduce_gate(tr.dres, y, NB, P, D, dgate, MODW, s));
        return dbias ? op->colsum_tiled(g_out, M, D, dbias, tr.red_ws, s) : 0;   // (dbias null: a LoRA handle, whose biases are frozen)
    }
    int final_layer(const float* v_pred, const float* v_target);
    int half_block(int i);
    int embedders();
};

// ---- phase 0: loss -> final projection -> final LayerNorm ----
int TrainBackward::final_layer(const float* v_pred, const float* v_target) {
    const float scale = 2.0f * tr.loss_scale / ((float)B * (float)(h->C * h->H * h->W));
    op = &h->ops(2 * L + 1);
    const int Nf = round_up(h->Nfin, 64);   // width of dfo: the final projection's features padded to whole 64-column tiles (zeros: mse_bwd_patch)
    RET_IF(op->mse_bwd_patch(v_pred, v_target, B, T, h->C, h->H, h->W, h->p, scale, tr.dfo, Nf, h->err_flag, s));
    if (lora) {   // the final layer is frozen: the dX chain alone (the LayerNorm backward still fills its dmod chunks, which nothing reads)
        RET_IF(gemm_dx(tr.dfo, tr.fin.w->wT, D, Nf, EPI_F32, tr.dtmp, D));
        float* dmf = tr.dmod + (size_t)L * 12 * D;
        return ln_bwd(tr.dtmp, tr.res[4 * L], h->mod + (size_t)L * 12 * D + D, 0, dmf, dmf + D);
    }
    // db: column sums over the Nf-wide (zero-padded) dfo, only the first Nfin belong to the bias: sum into a scratch row first
    GTAV_CHECK_HIP(hipMemsetAsync(tr.dSc, 0, Nf * sizeof(float), s));
    RET_IF(op->colsum_tiled(tr.dfo, M, Nf, tr.dSc, tr.red_ws, s));
    RET_IF(launch_add_f32(tr.fin.b->grad, tr.dSc, tr.fin.b->grad, h->Nfin, s));
    // dW_final [Nfin][D] += dfo^T xnF   (M = Nfin rows of the Nf-row transposed operand)
    RET_IF(op->transpose_tiled(tr.dfo, M, Nf, tr.tA, s));
    RET_IF(op->transpose_tiled(tr.xnF, M, D, tr.tB, s));
    GemmParams q = gemm_params(tr.tA, Mp, tr.tB, h->Nfin, D, Mp);
    q.out = tr.fin.w->grad; q.ldo = D;
    RET_IF(op->gemm(q, EPI_RESID, s));
    // d xnF = dfo W_final  -> fp32 [M][D]
    RET_IF(gemm_dx(tr.dfo, tr.fin.w->wT, D, Nf, EPI_F32, tr.dtmp, D));
    const float* mf = h->mod + (size_t)L * 12 * D;
    float* dmf = tr.dmod + (size_t)L * 12 * D;
    RET_IF(ln_bwd(tr.dtmp, tr.res[4 * L], mf + D, 0, dmf, dmf + D));
    return ada_grads((size_t)L * 12 * D, 2 * D, tr.fin_ada.w, tr.fin_ada.b);
}

// ---- half-block i of phases 1 .. L (the blocks in reverse: temporal half-block, then spatial); tr.dres = d loss / d (residual state) ----
int TrainBackward::half_block(int i) {
    const gtav_dit::Train::HB& b = tr.hb[i];
    const gtav_dit::Train::HalfSlots& p = tr.hs[i];
    const float* mb = h->mod + (size_t)i * 6 * D;
    float* dmb = tr.dmod + (size_t)i * 6 * D;
    op = &h->ops(i);
    // r_{2i+2} = r_{2i+1} + gate_mlp y2
    float* const ws_fc2 = tr.red_ws, *const ws_out = tr.red_ws + (defer_bias ? (size_t)NB * D : 0), *const ws_fc1 = tr.red_ws + (defer_bias ? (size_t)2 * NB * D : 0);   // (not deferred: every reduction follows its partial sums at once and the regions may coincide)
    RET_IF(gate_bwd(b.y2, mb + 5 * D, dmb + 5 * D, tr.g_d, bias_grad(p.fc2), ws_fc2));
    RET_IF(linear_dw(p.fc2, tr.g_d, D, b.hh, Hp, 0));
    RET_IF(gemm_dx(tr.g_d, p.fc2.w->wT, Hp, D, EPI_F16_TILED, tr.g_h, Hp));
    if (defer_bias) {
        RET_IF(op->gelu_bwd_tiled_colsum(tr.g_h, b.u, tr.g_u, M, Hp, nullptr, ws_fc1, h->err_flag, s));
    } else if (g_fuse_gelu && colsum_workspace(round_up(M, 128), Hp) <= tr.red_ws_floats) {
        RET_IF(op->gelu_bwd_tiled_colsum(tr.g_h, b.u, tr.g_u, M, Hp, bias_grad(p.fc1), tr.red_ws, h->err_flag, s));   // (LoRA: null, the partial sums stay unread)
    } else {
        RET_IF(op->gelu_bwd_tiled(tr.g_h, b.u, tr.g_u, (size_t)round_up(M, 128) * Hp, h->err_flag, s));
        if (!lora) RET_IF(op->colsum_tiled(tr.g_u, M, Hp, p.fc1.b->grad, tr.red_ws, s));
    }
    RET_IF(linear_dw(p.fc1, tr.g_u, Hp, b.xnB, D, 1));
    RET_IF(gemm_dx(tr.g_u, p.fc1.w->wT, D, Hp, EPI_F32, tr.dtmp, D));
    RET_IF(ln_bwd(tr.dtmp, tr.res[2 * i + 1], mb + 4 * D, 1, dmb + 3 * D, dmb + 4 * D));
    // r_{2i+1} = r_{2i} + gate_msa y1
    f16* const g_o = tn_dw ? tr.g_d2 : tr.g_d;   // (the fc2 weight gradient above still reads g_d when the grouped launch is deferred without copies)
    RET_IF(gate_bwd(b.y1, mb + 2 * D, dmb + 2 * D, g_o, bias_grad(p.out), ws_out));
    RET_IF(linear_dw(p.out, g_o, D, b.ao, D, 2));
    RET_IF(gemm_dx(g_o, p.out.w->wT, D, D, EPI_F16, tr.dao, D));
    if (i % 2 == 0) RET_IF(op->attn_spatial_bwd(b.q, b.k, b.v, tr.dao, NB, h->heads, P, D, h->rope_s.cs_dev, tr.g_qkv, h->err_flag, s));
    else RET_IF(op->attn_temporal_bwd(b.q, b.k, tr.dao, B, P, D, T, h->maxT, h->rope_t.cs_dev, tr.g_qkv, h->err_flag, s));
    RET_IF(linear_dw(p.qkv, tr.g_qkv, 3 * D, b.xnA, D, 3));
    if (defer_bias && !lora) {
        const float* wsv[3] = {ws_fc2, ws_out, ws_fc1};
        float* dbv[3] = {p.fc2.b->grad, p.out.b->grad, p.fc1.b->grad};
        const int spv[3] = {NB, NB, gelu_bwd_colsum_splits(M)}, nv[3] = {D, D, Hp};
        RET_IF(launch_colsum_reduce_multi(wsv, dbv, spv, nv, 3, s));
    }
    RET_IF(flush_dw());
    RET_IF(gemm_dx(tr.g_qkv, p.qkv.w->wT, D, 3 * D, EPI_F32, tr.dtmp, D));
    RET_IF(ln_bwd(tr.dtmp, tr.res[2 * i], mb + D, 1, dmb, dmb + D));
    // a LoRA handle: the adaLN projections are frozen, and block 0 is the last bucket the data-parallel harness reduces (train.gradient_buckets), so the
    // overflow publish of the backward pass lands here, in a blocks.0 adapter gradient, at the end of the last half-block differentiated
    if (lora) return i == 0 ? launch_overflow_publish(h->err_flag, p.qkv.la->grad, s) : 0;
    // all six dmod chunks of this half-block are in place: its adaLN projection's gradients
    return ada_grads((size_t)i * 6 * D, 6 * D, p.ada.w, p.ada.b);
}

// ---- phase L + 1: patch embedding: r_0 = xp W_pe^T + b_pe ----
int TrainBackward::embedders() {
    if (lora) return 0;   // the patch embedding and the conditioning path are frozen (the overflow publish: half_block(0))
    const int ldhc = D + h->Apad;
    op = &h->ops(2 * L);
    RET_IF(launch_colsum_f32(tr.dres, D, M, D, tr.pe.b->grad, tr.red_ws, s));
    RET_IF(op->to_tiled(tr.dres, M, D, tr.g_d, h->err_flag, s));
    // dW_pe [D][F]: xp keeps its Kpe - F zero pad columns, the gradient (and with it the master and the moments) has none
    RET_IF(gemm_dw(tr.g_d, D, tr.xp, h->Kpe, tr.pe.w->grad, -1, tr.pe.w->C));
    // ---- the shared conditioning path (fp32, `rows` = B T rows): c = W_2 SiLU(W_0 e + b_0) + b_2 (+ W_ext a + b_ext), SiLU(c) feeds every adaLN
    // projection (their own gradients were taken block by block above) ----
    RET_IF(launch_ada_bwd_dx(tr.dmod, MODW, h->w_ada, D, rows, tr.dSc, tr.ada_part, s));
    RET_IF(launch_silu_bwd(tr.dSc, D, tr.cpre, D, tr.dc, D, rows, D, s));
    RET_IF(launch_colsum_f32(tr.dc, D, rows, D, tr.t2.b->grad, tr.red_ws, s));
    RET_IF(launch_gemm_tn_f32(tr.dc, D, h->HC, ldhc, rows, D, D, tr.t2.w->grad, D, s));
    if (tr.have_actions) {
        // (action dropout: b_ext reached the kept rows only; W_ext's gradient is right by itself, the dropped rows' action columns of HC are zero)
        if (tr.have_keep) RET_IF(launch_colsum_f32_keep(tr.dc, D, rows, D, tr.keep, T, tr.ext.b->grad, tr.red_ws, s));
        else RET_IF(launch_colsum_f32(tr.dc, D, rows, D, tr.ext.b->grad, tr.red_ws, s));
        RET_IF(launch_gemm_tn_f32(tr.dc, D, h->HC + D, ldhc, rows, D, h->A, tr.ext.w->grad, h->A, s));
    }
    RET_IF(launch_gemm_nn_f32(tr.dc, D, h->w_t2cat, ldhc, rows, D, D, tr.dh0, D, s));
    RET_IF(launch_silu_bwd(tr.dh0, D, tr.z0, D, tr.dz0, D, rows, D, s));
    RET_IF(launch_colsum_f32(tr.dz0, D, rows, D, tr.t0.b->grad, tr.red_ws, s));
    RET_IF(launch_gemm_tn_f32(tr.dz0, D, h->E, 256, rows, D, 256, tr.t0.w->grad, 256, s));
    // Last kernel of the backward pass: a saturated / non-finite fp16 store on THIS rank becomes +inf in the embedder bucket (the one the data-parallel
    // harness all-reduces last, train.gradient_buckets), so the skip decision of the optimizer step is the same on every rank (ops.h)
    return launch_overflow_publish(h->err_flag, tr.pe.b->grad, s);
}

extern "C" {

// Backward of loss = mean((v_pred[:, -1] - v_target)^2) through the forward saved by gtav_dit_train_forward.  Gradients are ADDED to the
// gradient arena (gtav_dit_zero_grad first), multiplied by the loss scale.
// Phases of the backward pass (gtav_dit_train_backward_phases): 0 = loss, final projection, final LayerNorm; 1 .. L = the blocks in
// reverse, phase p = block L - p (both half-blocks and the block's adaLN projection: after phase p every gradient named "blocks.<L-p>.*" is
// complete, so its slice of the arena can be all-reduced while the earlier blocks are still being differentiated); L + 1 = patch embedding
// and the shared conditioning path (t_embedder, external_cond).  tr.dres / tr.dmod carry the state from one phase to the next.
int gtav_dit_train_backward_phases(gtav_dit* h, const float* v_pred, const float* v_target, int32_t phase_begin, int32_t phase_end, void* stream) {
    GTAV_REQUIRE(h && v_pred && v_target, "train_backward: null argument");
    RET_IF(train_not_swapped(h, "train_backward"));
    GTAV_REQUIRE(h->tr.on && h->tr.have_fwd, "train_backward: no saved forward (gtav_dit_train_forward)");
    GTAV_REQUIRE(phase_begin >= 0 && phase_begin <= phase_end && phase_end <= h->L + 2, "train_backward: phases [%d, %d) outside [0, %d]", phase_begin, phase_end,
                 h->L + 2);
    TrainBackward bw(h, (hipStream_t)stream);
    const int L = h->L;
    if (phase_begin <= 0 && 0 < phase_end) RET_IF(bw.final_layer(v_pred, v_target));
    for (int i = 2 * L - 1; i >= 0; --i) {
        const int l = i / 2, phase = L - l;
        if (phase < phase_begin || phase >= phase_end) continue;
        // recompute mode: the activations of block l are rebuilt at the head of its phase (the last block's are still those of the forward)
        if (h->tr.recompute && h->tr.rc_block != l) RET_IF(train_rerun_block(h, l, bw.s));
        RET_IF(bw.half_block(i));
    }
    if (phase_begin <= L + 1 && L + 1 < phase_end) RET_IF(bw.embedders());
    return 0;
}

int gtav_dit_train_backward(gtav_dit* h, const float* v_pred, const float* v_target, void* stream) {
    GTAV_REQUIRE(h, "train_backward: null handle");
    return gtav_dit_train_backward_phases(h, v_pred, v_target, 0, h->L + 2, stream);
}

// Slice [offset, offset + count) of the gradient arena that holds the parameters whose names start with `prefix` (names are laid out in
// lexicographic order, so "blocks.7." is one contiguous slice): the buckets of an all-reduce overlapped with the backward pass.
int gtav_dit_train_param_range(gtav_dit* h, const char* prefix, int64_t* offset, int64_t* count) {
    GTAV_REQUIRE(h && prefix && offset && count && h->tr.on, "train_param_range: bad argument / training is not enabled");
    const size_t plen = strlen(prefix);
    int64_t off = -1, cnt = 0, last_end = -1;
    for (auto& kv : h->wt.slots) {
        Slot& sl = kv.second;
        if (!sl.grad || kv.first.compare(0, plen, prefix) != 0) continue;
        const int64_t o = sl.grad - h->tr.grad_arena, n = (int64_t)sl.R * sl.C;
        if (off < 0) off = o;
        GTAV_REQUIRE(last_end < 0 || o == last_end, "train_param_range: parameters with prefix '%s' are not contiguous in the arena", prefix);
        last_end = o + n;
        cnt += n;
    }
    if (off < 0 && h->tr.lora.rank) { *offset = 0; *count = 0; return 0; }   // a frozen prefix of a LoRA handle ("final_layer.", the embedders): an empty bucket
    GTAV_REQUIRE(off >= 0, "train_param_range: no trainable parameter starts with '%s'", prefix);
    *offset = off;
    *count = cnt;
    return 0;
}

// One optimizer step over every trainable parameter: global gradient norm -> clipping coefficient (folded with 1 / loss_scale; a
// non-finite norm skips the step) -> AdamW -> refreshed fp16 operand copies (W and W^T) of the GEMM weights.
int gtav_dit_adamw_step(gtav_dit* h, float lr, float beta1, float beta2, float eps, float weight_decay, float max_grad_norm, void* stream) {
    GTAV_REQUIRE(h && h->tr.on, "adamw_step: training is not enabled");
    RET_IF(train_not_swapped(h, "adamw_step"));
    hipStream_t s = (hipStream_t)stream;
    gtav_dit::Train& tr = h->tr;
    if (tr.mixed) RET_IF(launch_err_fold(h->err_flag, tr.range_words, 0, h->n_groups, s));   // (the bits of recompute mode's re-runs, raised after the forward's fold)
    RET_IF(launch_sumsq(tr.grad_arena, tr.grad_count, tr.sumsq_part, s));
    // overflow (non-finite norm, or a saturated fp16 gradient / activation recorded in the error word) skips the step on the device; the
    // Adam step count and its bias corrections live in ctl[4..6] and advance only with applied steps
    // (a handle with averaged weights: the decay of this applied step goes to ctl[7] beside the bias corrections)
    RET_IF(launch_clip_coef(tr.ctl, tr.sumsq_part, sumsq_parts(tr.grad_count), 1.0f / (tr.loss_scale * tr.grad_div), max_grad_norm, beta1, beta2, tr.ema_decay,
                            tr.ema_warmup, h->err_flag, s));
    // one launch per operand type in use (one, unless a mixed-capable handle has groups of both): AdamW on every parameter + the 2-byte W / W^T operands of the
    // GEMM weights rewritten from the updated masters in their group's type.  The work items are independent, so the split changes no bit.
    // A handle with averaged weights runs the instantiation that also moves the shadow towards the master it just wrote (train.hip ADAM_STEP_EMA).
    for (int ty = 0; ty < 2; ++ty)
        if (tr.adam_n[ty]) {
            const OperandOps& o = operand_ops(ty != 0);
            RET_IF((tr.ema_decay > 0.f ? o.adamw_multi_ema : o.adamw_multi)(tr.adam_params, tr.adam_items + (ty ? tr.adam_n[0] : 0), tr.adam_n[ty], tr.ctl, lr, beta1,
                                                                           beta2, eps, weight_decay, s));
        }
    // a LoRA handle: the step moved the adapters only; every adapted weight's two images = clamp(W0 + s B A) again, one launch over all their tiles
    if (tr.lora.rank) RET_IF(train_lora_merge_all(h, s));
    RET_IF(launch_add_f32(h->b_t2, h->b_ext, h->b_t2a, h->D, s));   // fused bias of c when actions are given (gtav_dit_finalize)
    h->prepared.valid = false;
    h->kvrec.valid = false;
    return 0;
}

}  // extern "C"

// ---- mixed operand types on a training handle (gtav_dit_train_allow_mixed) ----
// The device list of AdamW work items, partitioned by the type their launch runs on: the items of fp16 groups' GEMM weights first, then those of bf16 groups'.
// The fp32 parameters have no 2-byte image and give the same bits on either twin: they ride with the fp16 part, or with the bf16 part when no group is fp16.
static int train_partition_items(gtav_dit* h) {
    gtav_dit::Train& tr = h->tr;
    bool any_f16 = false;
    for (unsigned char b : h->grp_bf16) any_f16 |= b == 0;
    std::vector<AdamItem> part[2];
    for (const AdamItem& it : tr.adam_items_host) {
        const Slot* sl = tr.params[it.param];
        part[sl->kind == SLOT_F16_PAD ? (sl->bf16 ? 1 : 0) : (any_f16 ? 0 : 1)].push_back(it);
    }
    tr.adam_n[0] = (int)part[0].size(); tr.adam_n[1] = (int)part[1].size();
    part[0].insert(part[0].end(), part[1].begin(), part[1].end());
    GTAV_REQUIRE((int)part[0].size() == tr.adam_n_items, "train_set_group_dtype: the optimizer's work items do not add up");
    GTAV_CHECK_HIP(hipMemcpy(tr.adam_items, part[0].data(), part[0].size() * sizeof(AdamItem), hipMemcpyHostToDevice));
    return 0;
}

// groups [g0, g1) of an enabled mixed-capable handle to `bf16`: launcher sets, W / W^T images from the fp32 masters, optimizer partition.  Returns the number changed.
static int train_switch_groups(gtav_dit* h, int g0, int g1, bool bf16, hipStream_t s, int* n_changed) {
    int changed = 0;
    for (int g = g0; g < g1; ++g) {
        if ((h->grp_bf16[g] != 0) == bf16) continue;
        h->grp_bf16[g] = bf16;
        ++changed;
        for (auto& kv : h->wt.slots) {
            Slot& sl = kv.second;
            if (sl.kind != SLOT_F16_PAD || sl.group != g) continue;
            sl.bf16 = bf16;
            if (!sl.set) continue;   // (no weight sent yet: gtav_dit_set_weight converts into the slot's type)
            GTAV_REQUIRE(sl.master, "train_set_group_dtype: '%s' has no fp32 master", kv.first.c_str());
            // what WeightTable::set does with the caller's fp32 tensor, from the master (contiguous [R][C])
            RET_IF(operand_ops(bf16).convert_pad(sl.master, sl.C, sl.R, sl.C, (f16*)sl.dst, sl.Rp, sl.Cp, 1.0f, 1, s, h->tr.range_words + g));
            if (sl.wT) RET_IF(operand_ops(bf16).convert_T(sl.master, sl.C, sl.R, sl.C, sl.wT, s));
        }
    }
    *n_changed = changed;
    if (!changed) return 0;
    h->any_bf16 = false;
    for (unsigned char b : h->grp_bf16) h->any_bf16 |= b != 0;
    // the saved activations of the last forward are of the old type, and so are the temporal K/V caches and whatever a captured step holds
    h->tr.have_fwd = false;
    h->tr.rc_block = -1;
    h->prepared.valid = false;
    h->kvrec.valid = false;
    h->drop_graphs();
    GTAV_CHECK_HIP(hipStreamSynchronize(s));   // (the re-partition below is a synchronous copy over a list an optimizer step in flight may still read)
    return train_partition_items(h);
}

static int train_mixed_handle(gtav_dit* h, const char* who) {
    GTAV_REQUIRE(h, "%s: null handle", who);
    GTAV_REQUIRE(h->tr.on, "%s: training is not enabled", who);
    GTAV_REQUIRE(h->tr.mixed, "%s: this training handle has one operand type for every group; opt in with gtav_dit_train_allow_mixed between gtav_dit_create and "
                 "gtav_dit_train_enable", who);
    return 0;
}

extern "C" {

int gtav_dit_train_set_group_dtype(gtav_dit* h, int32_t group, int32_t dtype, void* stream) {
    RET_IF(train_mixed_handle(h, "train_set_group_dtype"));
    RET_IF(train_not_swapped(h, "train_set_group_dtype"));
    GTAV_REQUIRE(dtype == GTAV_OPERAND_F16 || dtype == GTAV_OPERAND_BF16, "train_set_group_dtype: dtype %d (0 = fp16, 1 = bf16)", dtype);
    GTAV_REQUIRE(group >= -1 && group < h->n_groups, "train_set_group_dtype: group %d outside [-1, %d)", group, h->n_groups);
    int n = 0;
    return train_switch_groups(h, group < 0 ? 0 : group, group < 0 ? h->n_groups : group + 1, dtype == GTAV_OPERAND_BF16, (hipStream_t)stream, &n);
}

// the sticky words: copied back, cleared on the device
int gtav_dit_train_range_words(gtav_dit* h, int32_t* words_host, void* stream) {
    RET_IF(train_mixed_handle(h, "train_range_words"));
    GTAV_REQUIRE(words_host, "train_range_words: null argument");
    hipStream_t s = (hipStream_t)stream;
    static_assert(sizeof(int32_t) == sizeof(int), "the error words are 32-bit");
    GTAV_CHECK_HIP(hipMemcpyAsync(words_host, h->tr.range_words, (size_t)h->n_groups * sizeof(int), hipMemcpyDeviceToHost, s));
    GTAV_CHECK_HIP(hipStreamSynchronize(s));
    GTAV_CHECK_HIP(hipMemsetAsync(h->tr.range_words, 0, (size_t)h->n_groups * sizeof(int), s));
    return 0;
}

// Switch first, report afterwards: *n_switched and gtav_dit_get_operand_dtype are final when the call returns, with or without an error, so a caller that
// reads the types back after EVERY return agrees with the handle.  (Reporting first would clear the words and return before the switch: the host would hold
// an error, the handle its old types, and the saturation would come back with the next step.)
int gtav_dit_train_autorange(gtav_dit* h, const int32_t* merged_words_host, int32_t* n_switched, void* stream) {
    RET_IF(train_mixed_handle(h, "train_autorange"));
    RET_IF(train_not_swapped(h, "train_autorange"));
    GTAV_REQUIRE(n_switched, "train_autorange: null argument");
    *n_switched = 0;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> sticky(h->n_groups, 0);
    if (merged_words_host) sticky.assign(merged_words_host, merged_words_host + h->n_groups);
    else RET_IF(gtav_dit_train_range_words(h, sticky.data(), stream));
    // every other word, as gtav_dit_check reads them: the handle's, the inference bits gtav_dit_zero_grad set aside, the group words
    std::vector<int> w(4 + h->n_groups, 0);
    GTAV_CHECK_HIP(hipMemcpyAsync(w.data(), h->err_flag, w.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    GTAV_CHECK_HIP(hipStreamSynchronize(s));
    GTAV_CHECK_HIP(hipMemsetAsync(h->err_flag, 0, w.size() * sizeof(int), s));
    int other = w[0] | w[1];
    for (int g = 0; g < h->n_groups; ++g) {
        other |= w[4 + g];
        const bool switch_it = (sticky[g] & ERR_F16_SAT) && !h->grp_bf16[g];
        // a saturation bit of a group that is bf16 already is a fault (the twins never raise it for a finite value), not something to drop
        other |= switch_it ? sticky[g] & ~ERR_F16_SAT : sticky[g];
        if (switch_it) {
            int n = 0;
            RET_IF(train_switch_groups(h, g, g + 1, true, s, &n));
            *n_switched += n;
        }
    }
    return report_err_flag(other, "DiT training");
}

// ctl: [0] sum of squares of the scaled gradients, [1] step coefficient (0 = the step was skipped), [2] skipped steps so far,
// [3] unscaled global gradient norm of the last step (torch.nn.utils.clip_grad_norm_'s return value)
// Optimizer state of one parameter (AdamW first / second moments, contiguous in the parameter's state-dict shape) and the step counters:
// with gtav_dit_get_weight / set_weight (the fp32 masters) this is everything `accelerator.save_state` / `load_state` keep for the
// optimizer (train_dit.py:765-849).
static int opt_slot(gtav_dit* h, const char* name, int64_t numel, Slot** out) {
    GTAV_REQUIRE(h && name && h->tr.on, "opt_state: training is not enabled");
    auto it = h->wt.slots.find(name);
    GTAV_REQUIRE(it != h->wt.slots.end() && it->second.trainable && it->second.am && it->second.av, "opt_state: '%s' is not a trainable parameter", name);
    GTAV_REQUIRE(numel == (int64_t)it->second.R * it->second.C, "opt_state: '%s' has %d x %d elements, got %lld", name, it->second.R, it->second.C, (long long)numel);
    *out = &it->second;
    return 0;
}
int gtav_dit_get_opt_state(gtav_dit* h, const char* name, float* m_dst, float* v_dst, int64_t numel, void* stream) {
    Slot* sl = nullptr;
    RET_IF(opt_slot(h, name, numel, &sl));
    GTAV_REQUIRE(m_dst && v_dst, "get_opt_state: null destination");
    GTAV_CHECK_HIP(hipMemcpyAsync(m_dst, sl->am, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    GTAV_CHECK_HIP(hipMemcpyAsync(v_dst, sl->av, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
int gtav_dit_set_opt_state(gtav_dit* h, const char* name, const float* m_src, const float* v_src, int64_t numel, void* stream) {
    Slot* sl = nullptr;
    RET_IF(opt_slot(h, name, numel, &sl));
    GTAV_REQUIRE(m_src && v_src, "set_opt_state: null source");
    GTAV_CHECK_HIP(hipMemcpyAsync(sl->am, m_src, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    GTAV_CHECK_HIP(hipMemcpyAsync(sl->av, v_src, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
// The averaged weights of one trainable parameter, torch layout (the shadow is contiguous in the parameter's state-dict shape, like the moments).
static int ema_slot(gtav_dit* h, const char* who, const char* name, int64_t numel, Slot** out) {
    GTAV_REQUIRE(h && name && h->tr.on, "%s: training is not enabled", who);
    GTAV_REQUIRE(h->tr.ema_decay > 0.f, "%s: this handle keeps no averaged weights (gtav_dit_train_set_ema before gtav_dit_train_enable)", who);
    RET_IF(train_not_swapped(h, who));
    auto it = h->wt.slots.find(name);
    GTAV_REQUIRE(it != h->wt.slots.end() && it->second.trainable && it->second.ema, "%s: '%s' is not a trainable parameter", who, name);
    GTAV_REQUIRE(numel == (int64_t)it->second.R * it->second.C, "%s: '%s' has %d x %d elements, got %lld", who, name, it->second.R, it->second.C, (long long)numel);
    *out = &it->second;
    return 0;
}
int gtav_dit_get_ema(gtav_dit* h, const char* name, float* dst, int64_t numel, void* stream) {
    Slot* sl = nullptr;
    RET_IF(ema_slot(h, "get_ema", name, numel, &sl));
    GTAV_REQUIRE(dst, "get_ema: null destination");
    GTAV_CHECK_HIP(hipMemcpyAsync(dst, sl->ema, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
int gtav_dit_set_ema(gtav_dit* h, const char* name, const float* src, int64_t numel, void* stream) {
    Slot* sl = nullptr;
    RET_IF(ema_slot(h, "set_ema", name, numel, &sl));
    GTAV_REQUIRE(src, "set_ema: null source");
    GTAV_CHECK_HIP(hipMemcpyAsync(sl->ema, src, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}
// Masters <-> shadow, and the handle computes with what the masters now hold: one swap launch per operand type in use over the optimizer's own partition (the
// 2-byte images come out as a step that had produced those masters would have written them), then what the end of gtav_dit_adamw_step does.  Calling it again
// swaps back: the exchange moves fp32 words and the images are a function of the masters, so the handle is bit for bit where it was.
int gtav_dit_train_swap_ema(gtav_dit* h, void* stream) {
    GTAV_REQUIRE(h && h->tr.on, "train_swap_ema: training is not enabled");
    gtav_dit::Train& tr = h->tr;
    GTAV_REQUIRE(tr.ema_decay > 0.f, "train_swap_ema: this handle keeps no averaged weights (gtav_dit_train_set_ema before gtav_dit_train_enable)");
    GTAV_REQUIRE(h->finalized, "train_swap_ema: load the weights and finalize first");
    hipStream_t s = (hipStream_t)stream;
    for (int ty = 0; ty < 2; ++ty)
        if (tr.adam_n[ty]) RET_IF(operand_ops(ty != 0).adamw_swap_ema(tr.adam_params, tr.adam_items + (ty ? tr.adam_n[0] : 0), tr.adam_n[ty], s));
    if (tr.lora.rank) RET_IF(train_lora_merge_all(h, s));   // (the adapters were swapped: every adapted weight's images = clamp(W0 + s B A) of the ones in place)
    RET_IF(launch_add_f32(h->b_t2, h->b_ext, h->b_t2a, h->D, s));
    h->prepared.valid = false;
    h->kvrec.valid = false;
    tr.have_fwd = false;   // the saved activations are those of the other weights
    tr.rc_block = -1;
    tr.ema_swapped = !tr.ema_swapped;
    return 0;
}
int gtav_dit_get_opt_step(gtav_dit* h, int64_t* applied_steps, int64_t* skipped_steps, void* stream) {
    GTAV_REQUIRE(h && h->tr.on && applied_steps && skipped_steps, "get_opt_step: bad argument");
    float c[8];
    GTAV_CHECK_HIP(hipMemcpyAsync(c, h->tr.ctl, sizeof(c), hipMemcpyDeviceToHost, (hipStream_t)stream));
    GTAV_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    *applied_steps = (int64_t)c[4];
    *skipped_steps = (int64_t)c[2];
    return 0;
}
int gtav_dit_set_opt_step(gtav_dit* h, int64_t applied_steps, int64_t skipped_steps, void* stream) {
    GTAV_REQUIRE(h && h->tr.on && applied_steps >= 0 && applied_steps < (1 << 24) && skipped_steps >= 0, "set_opt_step: bad argument (the step count is kept as an exact fp32 integer: < 2^24)");
    float c[8];
    GTAV_CHECK_HIP(hipMemcpyAsync(c, h->tr.ctl, sizeof(c), hipMemcpyDeviceToHost, (hipStream_t)stream));
    GTAV_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    c[4] = (float)applied_steps; c[2] = (float)skipped_steps;
    GTAV_CHECK_HIP(hipMemcpy(h->tr.ctl, c, sizeof(c), hipMemcpyHostToDevice));
    return 0;
}
int gtav_dit_train_stats(gtav_dit* h, float* out4_host, void* stream) {
    GTAV_REQUIRE(h && out4_host && h->tr.on, "train_stats: bad argument");
    GTAV_CHECK_HIP(hipMemcpyAsync(out4_host, h->tr.ctl, 4 * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)stream));
    GTAV_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    return 0;
}

}  // extern "C"
