// host_setup_din.h -- the history stage of DIN / DIEN: k_dien_seq / k_dien_seq_mfma, k_din_pool's launch geometry, the attention tables
// of k_din_attn_cols / k_din_fused.
// Part of sparrow_hip.hip (one translation unit); included there, not compilable on its own.

// DIEN.py's sequence stage (GRU -> attention gate -> AUGRU).  Sixteen samples per wave on the matrix pipe (k_dien_mfma.h) where the shape
// allows: the host's packed image -> split-f16 MFMA A fragments with static scales from max|E| and the weights' row sums.  The
// lane-per-sample kernel stays (dien_frag = NULL, exact f32) for a non-finite table or weight, for a movie table the dynamic-range guard
// calls wide (an outlier row: s_xh and s_p come from max|E|, and [x ; h] share s_xh, so the ordinary rows AND the bounded state would lose
// their lo halves), and for weights k_dien_mfma_pack refuses (a block whose entries span more than 2^20).
int setup_dien_stage(sprk_engine* h, DevDin& d) {
    const sprk_plan& p = h->plan;
    const sprk_din& s = p.din;
    d.enabled = 1; d.T = s.T; d.hist_col = s.hist_col; d.cand_col = s.cand_col; d.row_stride = s.row_stride; d.vocab = s.vocab; d.hidden = s.hidden;
    const bool d10 = s.emb_dim == 10;
    const size_t img = d10 ? DienLayout<10, 32>::total_pad : DienLayout<16, 32>::total_pad;
    SPRK_TRY(need_bytes(h, s.table_slot, (size_t)s.vocab * s.row_stride * 4, "DIEN table"));
    SPRK_TRY(need_bytes(h, s.seq_slot, img * 4, "DIEN sequence weights"));
    d.table = (const float*)h->slot_ptr[s.table_slot];
    DienRun& r = h->dien_run;
    r.T = s.T; r.F = p.n_id_cols; r.hist_col = s.hist_col; r.cand_col = s.cand_col; r.Dp = s.row_stride; r.vocab = s.vocab; r.NA = p.n_aux;
    r.table = d.table;
    r.image = (const float*)h->slot_ptr[s.seq_slot];
    if (!h->tune.dien_mfma || !h->tune.dyn_f16 || s.hidden != 32 || (s.emb_dim != 10 && s.emb_dim != 16)) return SPRK_OK;
    h->dien_frag_floats = d10 ? DienFrag<10, 32>::total_pad : DienFrag<16, 32>::total_pad;
    const size_t ok_at = d10 ? DienFrag<10, 32>::S_OK : DienFrag<16, 32>::S_OK;
    // (open-coded, not static_scale: k_dien_mfma_pack reads max |E| from this device buffer and derives its scales there)
    DevScratch<unsigned> d_max;
    HIP_TRY(d_max.alloc(1));
    HIP_TRY(hipMemset(d_max.p, 0, sizeof(unsigned)));
    hipLaunchKernelGGL(k_v2_absmax, dim3(1024), dim3(256), 0, 0, d.table, (long long)s.vocab, s.row_stride, s.row_stride, d_max.p);
    HIP_TRY(hipGetLastError());
    float maxE = 0.f;
    HIP_TRY(hipMemcpy(&maxE, d_max.p, sizeof(float), hipMemcpyDeviceToHost));
    if (!(maxE < 3.0e38f)) return SPRK_OK;                    // NaN / Inf in the table
    bool wide = false;
    SPRK_TRY(wide_dynamic_range(d.table, (long long)s.vocab, s.row_stride, s.row_stride, maxE, &wide));
    if (wide) return SPRK_OK;
    const bool guard_on = h->tune.half_range_guard;
    float* frag = nullptr;
    SPRK_TRY(dev_alloc(h, &frag, h->dien_frag_floats * sizeof(float)));
    hipLaunchKernelGGL((d10 ? &k_dien_mfma_pack<10, 32> : &k_dien_mfma_pack<16, 32>), dim3(1), dim3(256), 0, 0, r.image, d_max.p, frag, guard_on ? 1 : 0);
    HIP_TRY(hipGetLastError());
    float ok = 0.f;
    HIP_TRY(hipMemcpy(&ok, frag + ok_at, sizeof(float), hipMemcpyDeviceToHost));
    if (ok == 1.f) h->dien_frag = frag;
    else dev_free(h, frag);
    return SPRK_OK;
}

// k_din_attn_cols / k_din_fused's tables, for the shapes of kDinVariants whose operands fit the split-f16 form: (W1+W2)^T and W4^T
// (k_din_prep_w), the per-id c-term table vc, the movie table pre-split into f16 hi / lo pairs, the cols kernel's A fragments.  Refused --
// the generic k_din_pool stays, and the tables made so far are released -- for non-finite weights, outlier rows, a split table beyond
// 32-bit offsets, and a W4 whose range does not fit the split.
// [kc - 1]; k_din_fused here in its attention-only forms (pooled vectors out; ATT: attention weights too) -- the TAIL forms: host_setup_din_tail.h
const DinColsKernels kDinColsKernels[2] = {{&k_din_attn_cols<1, false>, &k_din_attn_cols<1, true>}, {&k_din_attn_cols<2, false>, &k_din_attn_cols<2, true>}};
const DinFusedKernels kDinFusedAttnKernels[2] = {{&k_din_fused<1, false, false>, &k_din_fused<1, true, false>},
                                                 {&k_din_fused<2, false, false>, &k_din_fused<2, true, false>}};
const DinFusedKernel kDinFusedAttKernels[2] = {&k_din_fused<1, false, false, true>, &k_din_fused<2, false, false, true>};

int setup_din_attn(sprk_engine* h, const DevDin& d) {
    const sprk_plan& p = h->plan;
    const sprk_din& s = p.din;
    const int kc = (s.row_stride + 15) / 16, hc = s.hidden / 16, KP = kc * 16;
    const size_t vc_bytes = (size_t)s.vocab * s.hidden * sizeof(float), split_bytes = (size_t)s.vocab * KP * sizeof(float);
    if (s.T > 64 || vc_bytes >= ((size_t)4 << 30) || (size_t)s.vocab * s.row_stride * sizeof(float) >= ((size_t)4 << 30)) return SPRK_OK;   // 32-bit element offsets
    bool known = false;
    for (const DinVariant& dv : kDinVariants) known = known || (dv.kc == kc && dv.hc == hc && s.T <= dv.max_t);
    if (!known) return SPRK_OK;
    float *w12 = nullptr, *w4 = nullptr, *vc = nullptr, *tsplit = nullptr;
    auto refuse = [&]() {
        for (float* q : {w12, w4, vc, tsplit}) dev_free(h, q);
        h->derived_bytes -= vc_bytes + (tsplit ? split_bytes : 0);
        return SPRK_OK;
    };
    SPRK_TRY(dev_alloc(h, &w12, (size_t)s.hidden * KP * sizeof(float)));
    SPRK_TRY(dev_alloc(h, &w4, (size_t)s.hidden * KP * sizeof(float)));
    SPRK_TRY(dev_alloc(h, &vc, vc_bytes));
    h->derived_bytes += vc_bytes;
    hipLaunchKernelGGL(k_din_prep_w, dim3(8), dim3(256), 0, 0, d.W, s.hidden, s.row_stride, KP, 1.0f, w12, w4);
    HIP_TRY(hipGetLastError());
    // power-of-two scales from max|E|, max|W12|, max|W4|: |A_b| <= max|W12| + max|W4| max|E|
    // (the table by the rule of every static scale -- NaN / Inf, outlier rows: the ordinary rows would lose their lo halves; the two weight
    //  maxima enter a_scale as a sum with the table's and are only checked for NaN / Inf)
    float h_scale = 0.f, mxE = 0.f, mxW[2];
    SPRK_TRY(static_scale({{d.table, (long long)s.vocab, s.row_stride, s.row_stride, absmax_grid((long long)s.vocab * s.row_stride, 8192), 0}}, &h_scale, &mxE));
    SPRK_TRY(device_absmax({{w12, (long long)s.hidden, KP, KP, 4, 0}, {w4, (long long)s.hidden, KP, KP, 4, 1}}, mxW, 2));
    if (h_scale == 0.f || !(mxW[0] < 3.0e38f) || !(mxW[1] < 3.0e38f)) return refuse();
    const float a_scale = pow2_scale(mxW[0] + mxW[1] * mxE);
    hipLaunchKernelGGL(k_din_prep_w, dim3(8), dim3(256), 0, 0, d.W, s.hidden, s.row_stride, KP, a_scale, w12, w4);
    HIP_TRY(hipGetLastError());
    if (split_bytes >= ((size_t)4 << 30)) return refuse();
    SPRK_TRY(dev_alloc(h, &tsplit, split_bytes + 16));
    h->derived_bytes += split_bytes;
    long long sb = ((long long)s.vocab * KP + 255) / 256;
    if (sb > 65536) sb = 65536;
    hipLaunchKernelGGL(k_din_split_table, dim3((unsigned)sb), dim3(256), 0, 0, d.table, (long long)s.vocab, s.row_stride, KP,
                       h_scale, reinterpret_cast<_Float16*>(tsplit));
    HIP_TRY(hipGetLastError());
    long long blocks = ((long long)s.vocab * s.hidden + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_din_prep_vc, dim3((unsigned)blocks), dim3(256), 0, 0, d.W, d.bias, d.table, s.hidden, s.row_stride, (long long)s.vocab, vc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    // k_din_attn_cols: the weights as the static MFMA operand, sixteen samples per tile (k_din_cols.h), with scales that keep W4 * s4 and
    // h * c * sP inside f16's normal range.  U = a_scale h_scale (the accumulators' unit); sP = h_scale^2 2^-15 puts max |h c| sP in
    // [2^13, 2^15); W4 then carries s4 = U / sP = a_scale 2^15 / h_scale
    if (hc != 2 || (kc != 1 && kc != 2)) return refuse();
    const float rho = 32768.0f / h_scale;                     // s4 / a_scale
    float w4max = 0.f;                                        // max |W4| a_scale
    SPRK_TRY(device_absmax({{w4, (long long)s.hidden, KP, KP, 4, 0}}, &w4max, 1));
    const float w4s = w4max * rho;
    if (w4max != 0.f && !(w4s < 60000.0f && w4s >= 16.0f)) return refuse();
    float* frag = nullptr;
    SPRK_TRY(dev_alloc(h, &frag, 2 * 4 * 64 * 16 + 2 * 64 * 36 * sizeof(float)));
    float* coef = frag + 2 * 4 * 64 * 4;                      // behind the 8 KB of fragments
    hipLaunchKernelGGL(k_din_cols_coef, dim3(1), dim3(256), 0, 0, d.alpha, d.w2, s.T, coef);
    hipLaunchKernelGGL(k_din_cols_pack, dim3(1), dim3(256), 0, 0, w12, w4, KP, 1.0f, rho, reinterpret_cast<_Float16*>(frag));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    DinColsRun& c = h->din_cols_run;
    memset(&c, 0, sizeof(c));
    c.T = s.T; c.F = p.n_id_cols; c.hist_col = s.hist_col; c.cand_col = s.cand_col; c.Dp = s.row_stride; c.vocab = s.vocab;
    c.b2 = s.b2; c.acc_scale = a_scale * h_scale; c.unscale = 1.0f / (a_scale * h_scale); c.inv_h_scale = 1.0f / h_scale;
    c.kappa = 1.0f / 32768.0f;
    c.tsplit = tsplit; c.vc = vc; c.alpha = d.alpha; c.w2 = d.w2; c.frag = frag;
    c.coef = coef; c.idp = p.n_id_cols;
    const int lds_max = (2 * 64 * 36 + DC_WAVES * 16 * p.n_id_cols + DC_WAVES * 2 * 64 * 8) * 4;
    if (lds_max > 160 * 1024) return fail(SPRK_EINVAL, "DIN attention needs %d bytes of LDS", lds_max);
    h->din_cols_kernels = kDinColsKernels[kc - 1];
    SPRK_TRY(set_max_lds(h->din_cols_kernels.one, lds_max));
    SPRK_TRY(set_max_lds(h->din_cols_kernels.many, lds_max));
    h->din_cols_kc = kc;
    // k_din_fused (k_din_fused.h) takes the same tables; its tail half is set up by setup_din_tail
    // (a trip of its slot loop is four slots: for the reference's own hist_len = 5 that is 8 slots of work for 5, and
    // k_din_attn_cols' three-slot trips measure 10.7 us against 12.5 -- so short histories stay there)
    if (!h->tune.din_fused || s.T < h->tune.din_fused_min_t) return SPRK_OK;
    DinFusedRun& f = h->din_fused_run;
    memset(&f, 0, sizeof(f));
    f.T = c.T; f.F = c.F; f.hist_col = c.hist_col; f.cand_col = c.cand_col; f.Dp = c.Dp; f.vocab = c.vocab;
    f.b2 = c.b2; f.acc_scale = c.acc_scale; f.unscale = c.unscale; f.inv_h_scale = c.inv_h_scale; f.kappa = c.kappa;
    f.tsplit = c.tsplit; f.vc = c.vc; f.frag = c.frag; f.coef = c.coef; f.idp = c.idp;
    const int lds_attn = (DF_COEF_FLOATS + DF_WAVES * 16 * p.n_id_cols + DF_WAVES * 2 * 64 * 8) * 4;
    if (lds_attn > 160 * 1024) return SPRK_OK;
    h->din_fused_kernels[0] = kDinFusedAttnKernels[kc - 1];
    h->din_fused_att_kernel = kDinFusedAttKernels[kc - 1];
    SPRK_TRY(set_max_lds(h->din_fused_kernels[0].one, lds_attn));
    SPRK_TRY(set_max_lds(h->din_fused_kernels[0].many, lds_attn));
    SPRK_TRY(set_max_lds(h->din_fused_att_kernel, lds_attn));
    h->din_fused_attn = true;
    return SPRK_OK;
}

// DIN's attention stage: the generic k_din_pool for every shape (about 256 (sample, slot) rows in LDS per workgroup pass), and [r6]
// k_din_attn_cols / k_din_fused where setup_din_attn takes the shape -- SPRK_DIN_HALF=0 / SPRK_DIN_COLS=0 / SPRK_DIN_LEGACY=1 keep
// k_din_pool (until round 6 k_din_attn took those).
int setup_din_stage(sprk_engine* h, DevDin& d) {
    const sprk_din& s = h->plan.din;
    d.enabled = 1; d.T = s.T; d.hist_col = s.hist_col; d.cand_col = s.cand_col; d.row_stride = s.row_stride; d.vocab = s.vocab; d.hidden = s.hidden; d.b2 = s.b2;
    SPRK_TRY(need_bytes(h, s.table_slot, (size_t)s.vocab * s.row_stride * 4, "DIN table"));
    SPRK_TRY(need_bytes(h, s.w_slot, (size_t)s.hidden * 4 * s.row_stride * 4, "DIN att0 kernel"));
    SPRK_TRY(need_bytes(h, s.b_slot, (size_t)s.hidden * 4, "DIN att0 bias"));
    SPRK_TRY(need_bytes(h, s.alpha_slot, (size_t)s.T * s.hidden * 4, "DIN alpha"));
    SPRK_TRY(need_bytes(h, s.w2_slot, (size_t)s.hidden * 4, "DIN att1 kernel"));
    d.table = (const float*)h->slot_ptr[s.table_slot];
    d.W = (const float*)h->slot_ptr[s.w_slot];
    d.bias = (const float*)h->slot_ptr[s.b_slot];
    d.alpha = (const float*)h->slot_ptr[s.alpha_slot];
    d.w2 = (const float*)h->slot_ptr[s.w2_slot];
    int ms = 256 / s.T;                                       // samples per workgroup pass
    if (ms < 1) ms = 1;
    if (ms > 64) ms = 64;
    h->din_ms = ms;
    const int hs = s.row_stride + 4;
    h->din_lds_bytes = ((size_t)ms * s.T * hs + (size_t)ms * hs + (size_t)ms * s.T) * sizeof(float);
    if (h->din_lds_bytes > 160 * 1024) return fail(SPRK_EINVAL, "DIN stage needs %zu bytes of LDS", h->din_lds_bytes);
    SPRK_TRY(set_max_lds(k_din_pool, h->din_lds_bytes));
    h->din_grid_cap = lds_grid_cap(h, h->din_lds_bytes);
    if (h->tune.din_legacy || !h->tune.din_half || !h->tune.din_cols) return SPRK_OK;
    return setup_din_attn(h, d);
}
