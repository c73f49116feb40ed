// Part of salnmf.hip's translation unit (included there, inside its extern "C" block; not a stand-alone header):
// the host logic of engines wider than one tile -- n_features > 96 (NB feature blocks of X and W), n_signatures > 64 (NC
// chunks of <= 64 signatures) or both.  One forward evaluation per feature block and one driver of the update passes
// over the (block b, chunk ci) grid serve all three; a regime is never named below, only NB > 1 and NC > 1 are asked
// where the two decompositions really differ:
//   NC > 1: P = H W is a sum over the chunks, so a block's ratio R_b = X_b / (H W_b) is formed FIRST, by a chain of
//           forward launches through e->PR, and the fused passes run on the given ratio (RGIVEN), once per chunk, each with
//           the geometry of its chunk's size.  Otherwise the fused pass reads the block of X and forms P itself.
//   NB > 1: U = R W^T is a sum over the blocks, accumulated through Uacc by the BLOCKED instantiation (ublock: first /
//           middle / last block, the last one's pass writes H); the numerators go to Gblk, compact [K][width] per block,
//           and W is finished from there (w_finish_blocked_kernel).  Otherwise the numerators go to e->red and the
//           ordinary tail applies them.
// An engine with signature chunks never has a rescale of H pending (salnmf_set_H_scale refuses it, the MvNMF line search
// flushes at once, such an engine is never left ahead), so its chains and passes read H as it is.

static inline int ublock_code(const salnmf_engine* e, int b) { return b == 0 ? 1 : (b == e->NB - 1 ? 3 : 2); }
// where the reduced numerators of a split engine live
static inline double* wide_numerators(const salnmf_engine* e) { return e->NB == 1 ? e->red : e->Gblk; }

static int wide_fused(salnmf_engine* e, const FusedSel& sel, const FusedParams& p) {
    if (launch_fused_inst(sel, p, e->grid, e->stream, nullptr, nullptr)) return fail("no kernel instantiation for KS=%d KTM=%d KR=%d", sel.KS, sel.KTM, sel.KR);
    HIPCK(hipGetLastError());
    return 0;
}
// the slabs of the pass just run -> G[K][V], and with do_tail the update of the K rows of W at Wrows from them
static int wide_reduce(salnmf_engine* e, double* G, int K, int V, double* Wrows, int n_given, int clip_mode, int do_tail) {
    TailParams t = tail_params(e, e->grid, G, n_given, clip_mode, do_tail, false);
    t.W = t.Wout = Wrows;
    t.K = K;
    t.V = V;
    hipLaunchKernelGGL(tail_kernel, dim3(K), dim3(TAIL_BLOCK), 0, e->stream, t);
    HIPCK(hipGetLastError());
    return 0;
}
// W from the reduced numerators (wide_numerators)
static int wide_apply_W(salnmf_engine* e, int n_given, int clip_mode) {
    if (e->NB == 1) return launch_tail(e, 0, e->red, n_given, clip_mode, 1);
    hipLaunchKernelGGL(w_finish_blocked_kernel, dim3(e->K), dim3(256), 0, e->stream, e->Gblk, e->red, e->W, e->W, e->V, e->K, n_given, clip_mode);
    HIPCK(hipGetLastError());
    return 0;
}

// ---- forward: chunk ci's share of feature block b
//   W, hscale (MvNMF line-search trials): the signature matrix instead of e->W, and H read as clip(H * hscale[k]) -- both
//   compact over all signatures
static FwdParams chunk_fwd_params(salnmf_engine* e, const salnmf_engine::Chunk& c, int ci, const double* W, const double* hscale, int b) {
    FwdParams p{};
    p.X = e->X + (size_t)b * e->Np * VMAX;
    p.H = e->H + (size_t)ci * e->Np * e->KP;
    p.W = (W ? W : e->W) + (size_t)c.k0 * e->V + (size_t)VMAX * b;
    p.hscale = hscale ? hscale + c.k0 : nullptr;
    p.xlx = e->xlx ? e->xlx + (size_t)b * e->Np * 16 : nullptr;
    p.N = e->N;
    p.V = block_width(e, b);
    p.ldw = e->V;
    p.K = c.K;
    p.ntiles = e->ntiles;
    return p;
}
// the chain: chunks 0 .. NC-2 accumulate into e->PR (mode 2), the last chunk runs `last_mode` with `last` as its template
// (out, weights) on top of the accumulated product
static int chunk_chain(salnmf_engine* e, int last_mode, const FwdParams& last, const double* W, const double* hscale, int b) {
    for (int ci = 0; ci < e->NC; ++ci) {
        const auto& c = e->kc[(size_t)ci];
        FwdParams p = chunk_fwd_params(e, c, ci, W, hscale, b);
        p.pin = ci == 0 ? nullptr : e->PR;
        const bool is_last = ci == e->NC - 1;
        if (is_last) {
            p.wkl = last.wkl;
            p.wlh = last.wlh;
            p.out = last.out;
        } else {
            p.out = e->PR;
        }
        if (launch_forward_inst(c.KS, FWD_PIN + (is_last ? last_mode : 2), p, e->fgrid, e->stream, nullptr, nullptr))
            return fail("no forward instantiation for KS=%d", c.KS);
        HIPCK(hipGetLastError());
    }
    return 0;
}
// one forward evaluation of feature block b in mode 0, 1 or 2 (salnmf_forward_kernel.h) into t.out, with t's weights: a single
// launch on the block's slice of X, W and the x-only constants, or the chain over the signature chunks.
//   grid: workgroups of the single launch.  A chain always runs on e->fgrid; the only callers with another grid are the
//   narrow MvNMF steps (mv_fgrid), which a split engine never reaches (salnmf_host_mv.h: every entry point branches to the
//   plain form first), so a caller may take its partials to lie e->fgrid apart on every split engine.
static int wide_forward(salnmf_engine* e, int mode, const FwdParams& t, int b, const double* W, const double* hscale, int grid) {
    if (e->NC > 1) return chunk_chain(e, mode, t, W, hscale, b);
    FwdParams p = chunk_fwd_params(e, e->kc[0], 0, W, hscale, b);
    p.wkl = t.wkl;
    p.wlh = t.wlh;
    p.out = t.out;
    switch (mode) {  // (launch_forward is a template, and this file sits inside an extern "C" block)
        case 0: return launch_forward<0>(e, p, grid);
        case 1: return launch_forward<1>(e, p, grid);
        default: return launch_forward<2>(e, p, grid);
    }
}

// ---- the update passes over the (block, chunk) grid on the resident (W, H).  Per block: its ratio into e->PR (NC > 1), then
// per chunk at most ONE fused pass -- the chunk's numerator slabs (do_g, unless all its signatures are given), reduced
// behind the pass, and / or its share of the H update (do_u) -- then one exchange of the numerators between sample shards,
// then W (unless g_only: the caller takes its own root from wide_numerators, or applies them later).
//   Hout, hfloor: where the new H goes and its floor (CorrNMF: aux = H * U unclipped, H itself untouched).  Every block's
//   ratio is formed from the OLD H: with one chain (NB == 1) or none (NC == 1: only the last block's pass writes H, tile
//   by tile behind that tile's own numerator) Hout may be H itself; with a chain per block only an update_H alone may (the
//   last block's chain is done before its passes), a joint step writes the second buffer (wide_kl_step_once)
//   weighted = false: MvNMF's and CorrNMF's passes (no sample weights: mvnmf.py:56,162-165, corrnmf_det.py:80-85)
// h_pending is left to the callers: whoever had H rewritten in full clears it.  (The driver of engines with blocks AND
// chunks used to clear it itself, the one of chunks alone never did; both are no-ops -- see the head of this file.)
static int wide_passes(salnmf_engine* e, bool do_g, bool do_u, int n_given, int clip_mode, double* Hout, double hfloor, bool weighted, bool g_only) {
    const bool blocks = e->NB > 1, chunks = e->NC > 1;
    if (chunks && e->h_pending) return fail("internal: an engine with signature chunks has a rescale of H pending");
    const size_t hc = (size_t)e->Np * e->KP;
    const bool any_g = do_g && n_given < e->K;
    // one block and one shard: each chunk's reduction applies its rows of W on the spot
    const bool tail_applies = !blocks && !g_only && !sharded(e);
    for (int b = 0; b < e->NB; ++b) {
        const int vb = block_width(e, b);
        if (chunks) {
            FwdParams last{};
            last.out = e->PR;
            CK(chunk_chain(e, 4, last, nullptr, nullptr, b));
        }
        for (int ci = 0; ci < e->NC; ++ci) {
            const auto& c = e->kc[(size_t)ci];
            const int given = std::max(0, std::min(c.K, n_given - c.k0));  // given rows inside this chunk
            const bool g = do_g && given < c.K;
            if (!g && !do_u) continue;
            FusedParams p = fused_params(e);
            to_block(e, p, b);
            if (chunks) {
                p.X = e->PR;
                p.hscale = nullptr;
            }
            p.W += (size_t)c.k0 * e->V;
            p.K = c.K;
            p.H = p.Hout = e->H + (size_t)ci * hc;
            if (do_u) p.Hout = Hout + (size_t)ci * hc;
            p.hfloor = hfloor;
            if (!weighted) p.wkl = p.wlh = nullptr;
            if (blocks && do_u) {
                p.Uacc = e->Uacc + (size_t)ci * hc;
                p.ublock = ublock_code(e, b);
            }
            if (!chunks && !do_u) {
                // numerators alone from a block of X: the pass of the one-block engine, weighted only where weights are set
                CK((launch_fused<true, false, false>(e, p)));
            } else {
                CK(weight_arrays(e, p));  // (the BLOCKED and RGIVEN instantiations are the weighted-capable ones)
                FusedSel sel{c.KS, c.KTM, c.KR, g, do_u, false, true, false, blocks && do_u};
                sel.RGIVEN = chunks;
                CK(wide_fused(e, sel, p));
            }
            if (g) {
                double* G = blocks ? e->Gblk + (size_t)b * e->K * VMAX + (size_t)c.k0 * vb : e->red + (size_t)c.k0 * e->V;
                CK(wide_reduce(e, G, c.K, vb, e->W + (size_t)c.k0 * e->V, given, clip_mode, tail_applies ? 1 : 0));
            }
        }
    }
    // sample shards: the numerators lie back to back as K * V doubles in all (the blocks' compact ones, or the chunks' rows
    // of one K x V matrix): one exchange for all of them (the given rows' numerators were not formed: they are not read either)
    if (any_g && sharded(e)) CK(allreduce(e, wide_numerators(e), (size_t)e->K * e->V));
    if (any_g && !g_only && !tail_applies) CK(wide_apply_W(e, n_given, clip_mode));
    return 0;
}

// one joint step (update_WH, _utils_klnmf.py:281-361): both halves from the OLD (W, H)
static int wide_kl_step_once(salnmf_engine* e, int n_given) {
    const bool joint = n_given < e->K;  // else W untouched (:330-331)
    const bool second = joint && e->NB > 1 && e->NC > 1;  // (wide_passes: a chain per block reads the old H of all chunks)
    if (second) CK(ensure_halt(e));
    CK(wide_passes(e, joint, true, n_given, SALNMF_CLIP_ALL, second ? e->Halt : e->H, kEps, true, false));
    if (second) std::swap(e->H, e->Halt);
    e->h_pending = false;  // the new H was written in full
    return 0;
}
