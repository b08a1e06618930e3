// The split-f16 / single-f16 matrix field kernel.  Included by unerf_nerf.hip (section 5b'') TWICE, as two __global__
// templates of one text: UNERF_MFMA16_KERNEL = field_kernel_mfma16 (one frame per launch; UNERF_MFMA16_VIEWS = false) and
// views_kpass_kernel_mfma16 (XA = FieldViews: several views per launch, unerf_field_fwd_views; UNERF_MFMA16_VIEWS = true).
// Two names rather than one more instantiation: the single-view kernels stay the kernels they were, instruction for
// instruction, and the set of field_kernel* instantiations stays what field_launch() can launch (tests/test_isa_check_cpu.py).
template <int MODE, int TCNN, bool SITES = false, bool DROP = false, bool F1 = false, typename... XA>
// (the single-product K-pass kernel at 3 waves per SIMD was measured twice and lost both times: round 3, 168 VGPRs, 96 B of
// scratch, trunk operands re-read from LDS -- 4.84 vs 3.89 ms per launch, profiles/r3_exp_f16_single_occ3.json; round 7,
// 163 VGPRs, no scratch, the SH k-step of colour 0 recomputed per pass -- 12.71 - 12.88 vs 12.44 - 12.56 ms, docs/experiments.md 7.1)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((MODE == UNERF_FIELD_ACTIVE && TCNN != 1) ? 3 : 2)))
void UNERF_MFMA16_KERNEL(FieldArgs a, uint32_t num_tiles, FastDiv div_s, XA... xa) {
    constexpr bool XM = xa_is_keep<XA...>::value;
    constexpr bool VW = xa_is_views<XA...>::value;   // XA = FieldViews: several views in the launch (unerf_field_fwd_views)
    static_assert(XM || VW || sizeof...(XA) == 0, "trailing argument: KeepArgs, FieldViews or none");
    static_assert(VW == UNERF_MFMA16_VIEWS, "FieldViews rides on views_kpass_kernel_mfma16, and nothing else does");
    static_assert(!XM || (SITES && DROP && MODE == UNERF_FIELD_MCDROPOUT), "explicit keep masks ride on the general SITES path");
    static_assert(!VW || (!SITES && DROP && MODE == UNERF_FIELD_MCDROPOUT), "the views form exists where a per-view value is read: generated masks");
    extern __shared__ float lds[];
    const uint32_t* vkeys = nullptr;
    if constexpr (VW) {
        __shared__ uint32_t s_vkey[UNERF_NERF_MAX_VIEWS];
        if (threadIdx.x < UNERF_NERF_MAX_VIEWS) s_vkey[threadIdx.x] = vw_of(xa...).key[threadIdx.x];
        vkeys = s_vkey;
    }
    {
        const float4* src = reinterpret_cast<const float4*>(a.p.mfma16_blob);
        float4* dst = reinterpret_cast<float4*>(lds);
        for (int i = threadIdx.x; i < (F1 ? UNERF_MFMA16_BLOB_FLOATS : UNERF_MFMA_BLOB_FLOATS) / 4; i += 256) dst[i] = src[i];
    }
    __shared__ uint32_t s_tl[TCNN ? MF_TL_WORDS : 1];
    if (TCNN) mf_stage_tcnn_levels<(TCNN == 2 ? 2 : 3)>(a, s_tl);
    __syncthreads();
    const int lane_c = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane_c & 31, h = lane_c >> 5;
    const int64_t N = a.R * (int64_t)a.S;
    const uint32_t mask = (1u << a.p.log2T) - 1u;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const uint32_t tpx = (num_tiles + 7u) / 8u;
    const uint32_t tile_end = (xcd + 1) * tpx < num_tiles ? (xcd + 1) * tpx : num_tiles;
    bool f1_bad = false;   // an f16 operand overflowed: F1 -- an output pre-activation of this lane was inf / NaN (see the
                           // epilogue); split form -- a colour layer's pre-activations were NaN (see colour 0 below)
    for (uint32_t tile = xcd * tpx + (uint32_t)slot * 4u + (uint32_t)wv; tile < tile_end; tile += (uint32_t)bpx * 4u) {
        int lane = lane_c;  // opaque per iteration: keeps the (tile-invariant) LDS operand reads inside the loop
        asm volatile("" : "+v"(lane));
        const TileSample ts = tile_sample(a, tile, div_s, j);
        const bool valid = ts.valid;
        const int64_t n = ts.n;
        const float dxr = ts.dx, dyr = ts.dy, dzr = ts.dz;
        float px = ts.px, py = ts.py, pz = ts.pz;
        const float sel = unerf_normalize_position(px, py, pz, a.box);
        // packed fp32x2 blend: this kernel has the registers for it (123 VGPRs without) in every mode
        // colour layer 0, SH half (pass-invariant): components 8h..8h+7 of this lane half, one k-step.  (A closure called
        // behind the gather: stated in line there, the same statements compile to other code in 36 of the kernels.)
        f32x16 csh0 = mf16_bias(lds, 3, h), csh1 = mf16_bias(lds, 4, h);
        auto sh_layer = [&]() {
            float sh[16];
            float ux = (dxr + 1.f) / 2.f, uy = (dyr + 1.f) / 2.f, uz = (dzr + 1.f) / 2.f;
            if (a.p.sh_remap) {
                ux = ux * 2.f - 1.f;
                uy = uy * 2.f - 1.f;
                uz = uz * 2.f - 1.f;
            }
            unerf_sh16(ux, uy, uz, sh);
            const uint32_t hm = 0u - (uint32_t)h;
            float mine[8];
#pragma unroll
            for (int q = 0; q < 8; ++q)
                mine[q] = __uint_as_float((__float_as_uint(sh[8 + q]) & hm) | (__float_as_uint(sh[q]) & ~hm));
            f16x8 bhi, blo;
            mf16_split8<F1>(mine, bhi, blo);
            mf16_mac2<F1>(lds, 10, 11, lane, bhi, blo, csh0, csh1);
        };
        u32x8 feat_pk;
        const f32x16 feat = mf_gather_feats<true, TCNN>(a, px, py, pz, h, mask, s_tl, &feat_pk);
        sh_layer();

        // layer 0: 32 -> 64 (this half's 16 features = two k-steps), ReLU; the 64 hidden units are the trunk
        // layer's four k-steps and do not depend on the MC pass: they are split into f16 operand quads ONCE
        f16x8 hhi[4], hlo[4];
        {
            f32x16 hid0 = mf16_bias(lds, 0, h), hid1 = mf16_bias(lds, 1, h);
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                f16x8 bhi, blo;
                mf16_feat_operand<TCNN, F1>(feat, feat_pk, st, bhi, blo);
                mf16_mac2<F1, TCNN == 2>(lds, 2 * st, 2 * st + 1, lane, bhi, blo, hid0, hid1);
            }
            if constexpr (F1) {   // ReLU on the packed halves (relu(cvt(x)) = cvt(relu(x)): mf16_split_relu), half the instructions
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    mf16_split_relu(st < 2 ? hid0 : hid1, st & 1, hhi[st]);
                    hlo[st] = hhi[st];
                }
            } else {
                hid0 = mf_relu(hid0);
                hid1 = mf_relu(hid1);
#pragma unroll
                for (int st = 0; st < 4; ++st) mf16_split<F1>(st < 2 ? hid0 : hid1, st & 1, hhi[st], hlo[st]);
            }
        }

        const int passes = (MODE == UNERF_FIELD_MCDROPOUT && a.p.K > 0) ? a.p.K : 1;
        // the trunk-out operands (4 k-steps x 2 quads = 32 VGPRs) kept in registers across the passes (-3.5 %); the
        // 16-row trunk-out layer of MCDROPOUT folded into two MFMAs per k-step (-1 % kernel time)
        constexpr bool TRUNK_RESIDENT = MODE == UNERF_FIELD_MCDROPOUT && DROP && !SITES;
        // F1: the first operand of a (folded or plain) trunk slab is W_hi, which is all the single-product form reads
        constexpr bool FOLD = MODE == UNERF_FIELD_MCDROPOUT && !F1;
        f16x8 ta0[4], ta1[4];   // first / second operand of trunk slab 4 + st
        if (TRUNK_RESIDENT) {
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                ta0[st] = *reinterpret_cast<const f16x8*>(lds + (4 + st) * 512 + lane * 4);
                if (!F1) ta1[st] = *reinterpret_cast<const f16x8*>(lds + (4 + st) * 512 + 256 + lane * 4);
            }
        }
        constexpr bool drop = DROP;   // host: a.drop_on
        const uint32_t sidx = (uint32_t)((uint64_t)a.ray_offset * (uint64_t)a.S + (uint64_t)n);
        uint32_t mk0[8], mk1[8], mk2[8], mk3[8];
        uint32_t base0_h0 = 0u;   // SITES only: the sample's base hash stays live across the passes
        const bool drop_trunk = SITES ? (drop && (a.drop_sites & UNERF_DROP_TRUNK)) : drop;
        const bool drop_head1 = SITES ? (drop && (a.drop_sites & UNERF_DROP_HEAD1)) : drop;
        if (drop && !XM) {
            uint32_t pre;
            if constexpr (VW) {   // the counter inside the sample's own frame, under its view's key
                const FieldViews& fv = vw_of(xa...);
                const uint32_t view = fastdiv((uint32_t)ts.r, fv.div_hw);
                pre = unerf_mc_pre(vkeys[view], ((uint32_t)ts.r - view * fv.hw) * (uint32_t)a.S + (uint32_t)ts.s);
            } else {
                pre = unerf_mc_pre(unerf_mc_key(a.p.seed, 0u), sidx);
            }
            const uint32_t base0 = unerf_mc_base_h(pre, (uint32_t)h);   // this lane half's
            if (SITES) base0_h0 = base0;
            mf_mask_init(mk0, 0, h, base0, 0u);
            mf_mask_init(mk1, 1, h, base0, 0u);
            mf_mask_init(mk2, 0, h, base0, 1u);
            mf_mask_init(mk3, 1, h, base0, 1u);
        }
        for (int k = 0; k < passes; ++k) {
            asm volatile("" : "+v"(lane));
            if constexpr (XM) {   // this pass' words from the keep bits instead of a generator step
                if (drop_trunk) {
                    mf_xm_words(mk0, xm_row(xm_of(xa...), 0, k, n), 0, h);
                    mf_xm_words(mk1, xm_row(xm_of(xa...), 0, k, n), 1, h);
                }
                if (drop_head1) {
                    mf_xm_words(mk2, xm_row(xm_of(xa...), 2, k, n), 0, h);
                    mf_xm_words(mk3, xm_row(xm_of(xa...), 2, k, n), 1, h);
                }
            } else if (drop && k > 0) {
                mf_mask_step(mk0);
                mf_mask_step(mk1);
                mf_mask_step(mk2);
                mf_mask_step(mk3);
            }
            // [probe:kpass-pass-start]
            // Wave priority: low through the matrix layers of a pass, high from the rgb layer to the end of the pass --
            // and, after the last pass, through the next tile's gathers.  The tail (packed-fma chains, the half exchange,
            // exp / rcp, stores) and the gather prologue are short instruction streams that wait on latencies; letting
            // them go first when both waves of a SIMD are ready takes 4.2 % off the K = 8 kernel (same box, six
            // placements tried: benchmarks/multi_ab.sh, profiles/r2_exp_setprio.json); high priority for the matrix
            // layers instead gives 1.3 %, for the prologue alone nothing.
            __builtin_amdgcn_s_setprio(0);
            // trunk out: 64 -> out1 rows (row 0 density, 1..15 geo, 16 beta) from the (masked) hidden operands
            f32x16 t = mf16_bias(lds, 2, h);
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                f16x8 bhi = hhi[st], blo = hlo[st];
                if (drop_trunk) mf16_apply_masks<F1>(bhi, blo, st < 2 ? mk0 : mk1, st & 1, a.keep_pk);
                f16x8 a0, a1;
                if (TRUNK_RESIDENT) {
                    a0 = ta0[st];
                    a1 = F1 ? ta0[st] : ta1[st];
                } else {
                    a0 = mf16_lds_op(lds + (4 + st) * 512 + lane * 4);
                    a1 = F1 ? a0 : *reinterpret_cast<const f16x8*>(lds + (4 + st) * 512 + 256 + lane * 4);
                }
                if (F1) {
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, bhi, t, 0, 0, 0);
                } else if (FOLD) {
                    t = mf16_mac_fold_ops(a0, a1, bhi, blo, t);
                } else {   // a0 = W_hi, a1 = W_lo: small terms first
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, bhi, t, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, blo, t, 0, 0, 0);
                    t = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, bhi, t, 0, 0, 0);
                }
            }
            if (FOLD) t = mf16_fold_rows(t);
            // colour 0: geo rows of t (registers 0..7 = one k-step) on top of the SH partial sum, ReLU
            f32x16 c0 = csh0, c1 = csh1;
            {
                f16x8 bhi, blo;
                mf16_split<F1>(t, 0, bhi, blo);
                mf16_mac2<F1>(lds, 8, 9, lane, bhi, blo, c0, c1);
            }
            if (!F1) {   // F1: ReLU on the packed f16 operands instead (mf16_split_relu: half the instructions)
                // Split form: an activation beyond 65504 is carried as hi = +inf, lo = -inf, and EVERY unit of the layer it
                // feeds becomes inf - inf = NaN.  Trunk overflows reach the density logit as NaN and are caught by the
                // composite kernels; behind a ReLU they would not be -- the integer maximum below maps a NaN whose sign bit
                // is set to 0, and the layers after it then see a plausible all-zero hidden vector.  So one accumulator of
                // each colour layer is tested before its ReLU (all 64 are NaN or none): two compares per pass.
                f1_bad |= c0[0] != c0[0];
                c0 = mf_relu(c0);
                c1 = mf_relu(c1);
            }
            // colour 1: 64 -> 64, ReLU
            f32x16 d0 = mf16_bias(lds, 5, h), d1 = mf16_bias(lds, 6, h);
            if (SITES && drop && (a.drop_sites & UNERF_DROP_HEAD0)) {   // rgb_dropout_layers contains 1 (non-default): masks on c
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    f16x8 bhi, blo;
                    if (F1) mf16_split_relu(st < 2 ? c0 : c1, st & 1, bhi);
                    else mf16_split<F1>(st < 2 ? c0 : c1, st & 1, bhi, blo);
                    uint32_t mw[8];
                    if constexpr (XM) mf_xm_words(mw, xm_row(xm_of(xa...), 1, k, n), st >> 1, h);
                    else mf_mask_words_at(mw, st >> 1, h, base0_h0, 2u, k);
                    mf16_apply_masks<F1>(bhi, blo, mw, st & 1, a.keep_pk);
                    mf16_mac2<F1>(lds, 12 + 2 * st, 12 + 2 * st + 1, lane, bhi, blo, d0, d1);
                }
            } else {
                mf16_layer64<2, F1, F1>(lds, 12, lane, c0, c1, d0, d1);
            }
            // (F1 with this layer as four more k-steps on the matrix pipe -- 16 conversions + 16 packed ReLUs + 48 packed-mask
            // instructions + 4 MFMAs instead of the 154 instructions below -- was built and measured: 3.68 vs 3.89 ms per
            // launch, but the f16 rounding of the last layer's operands moved one MC-dropout AUSE figure past its 1e-3
            // gate; profiles/r3_exp_f16_rgb_on_mfma.json, DESIGN.md 4.5.  The colour layer stays fp32 in every form.)
            float o[3];
            if constexpr (F1) {
                // colour 2: 64 -> 3 as four more k-steps on the matrix pipe (rows 0..2 of one 32-row block; slabs behind the
                // fp32 tail of the blob), its operands = the hidden units rounded to f16 -- which is what the reference's
                // Linear computes under its forced autocast (mcdropout_models.py:86-92: f16 inputs and weights, fp32
                // accumulate) and what tcnn's FullyFusedMLP does.  ReLU and the dropout masks ride on the packed halves like
                // the trunk's: convert 0.5 + ReLU 0.5 + mask 1.5 instructions per unit instead of ReLU 1 + compare 1 +
                // select 1 on the fp32 accumulators, and 4 MFMAs (128 issue cycles) instead of 48 packed FMAs + the half
                // exchange.  (Round 3 measured this form at -5 % and dropped it over ONE AUSE figure at 1.04e-3 -- a gate
                // that the reference's own two arithmetics miss by more on that target, DESIGN.md 6.)
                __builtin_amdgcn_s_setprio(1);
                f32x16 o4;
#pragma unroll
                for (int r = 0; r < 16; ++r) o4[r] = 0.f;
#pragma unroll
                for (int st = 0; st < 4; ++st) {
                    f16x8 bhi;
                    if (drop_head1) {
                        const uint32_t (&w)[8] = st < 2 ? mk2 : mk3;
                        u32x4 dd;
#pragma unroll
                        for (int p = 0; p < 4; ++p) dd[p] = mf16_keep_diff(w[4 * (st & 1) + p], a.keep_pk);
                        mf16_split_relu_drop(st < 2 ? d0 : d1, st & 1, dd, bhi);
                    } else {
                        mf16_split_relu(st < 2 ? d0 : d1, st & 1, bhi);
                    }
                    const f16x8 aw = mf16_lds_op(lds + UNERF_MFMA_BLOB_FLOATS + st * 256 + lane * 4);
                    o4 = __builtin_amdgcn_mfma_f32_32x32x16_f16(aw, bhi, o4, 0, 0, 0);
                }
                // rows 0..2 = registers 0..2 of the h = 0 half: one v_permlane32_swap each hands them to both halves
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(o4[c]), __float_as_uint(o4[c]), false, false);
                    o[c] = __uint_as_float(sw[0]) + lds[MF_H2_OFF + 192 + c];
                }
            } else {
            if (!F1) f1_bad |= d0[0] != d0[0];
            d0 = mf_relu(d0);
            d1 = mf_relu(d1);
            if (drop_head1) {   // masks on the fp32 accumulators: one half-word compare + one select per unit
                d0 = mf_dropout_keep(d0, mk2, a.keep_hi);
                d1 = mf_dropout_keep(d1, mk3, a.keep_hi);
            }
            __builtin_amdgcn_s_setprio(1);
            // colour 2: 64 -> 3 on the VALU in fp32 (weights pre-scaled by the dropout scale when masks are on).
            // A SIMD has an issue lane (4 cycles per VALU instruction, ~10 per f16 MFMA) beside its matrix lane (32 per MFMA:
            // benchmarks/issue_sweep_probe.hip, DESIGN.md 4.4), and these kernels are bound by the issue lane, so a layer belongs
            // where it costs fewer ISSUE cycles: as four more k-steps on the matrix pipe this one took 12 MFMAs + 48 split
            // instructions (~310 issue cycles, 29 of 32 output rows wasted), as packed fp32 FMAs it takes 48 + the half-to-half
            // exchange (~220).  (Rounds 2 - 5 argued the same choice from "MFMA and VALU never overlap, 32 + 4 cycles".)
            {
                const float4* wq = reinterpret_cast<const float4*>(lds + MF_H2_OFF + h * 48);
                // Per 32-unit block the 12 weight quads (3 channels x 4) are read into an array FIRST and the 24 packed FMAs
                // follow.  Written as one load per use the compiler issued each ds_read_b128 directly in front of its two FMAs
                // and waited for it: 24 exposed LDS round trips per pass (`D1 W1 v1 n0 v1` 24 times in the listing), in which
                // both waves of a SIMD tended to sit at once -- the K-pass "f16" kernel went 16.2 -> 15.0 ms per launch with the
                // reads grouped (profiles/r4_exp_rgb_weight_reads_*.json).  Forcing the grouping further with
                // sched_group_barrier was slower, and issuing the three channels' chains interleaved (no `s_nop` between
                // dependent packed FMAs, 439 instead of 476 instructions per pass) changed nothing: the other wave fills
                // those slots (profiles/r4_exp_rgb_interleave_*.json).
                // (the split form has no registers for 12 quads in flight -- 28 B of scratch with them -- and groups 4)
                constexpr int CG = F1 ? 3 : 1;   // channels whose weights are read together
                unerf_v2f acc2[3] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
                for (int blk = 0; blk < 2; ++blk) {
                    const f32x16& dv = blk ? d1 : d0;
#pragma unroll
                    for (int c0g = 0; c0g < 3; c0g += CG) {
                        float4 wv[CG][4];
#pragma unroll
                        for (int c = 0; c < CG; ++c)
#pragma unroll
                            for (int q4 = 0; q4 < 4; ++q4) wv[c][q4] = wq[blk * 24 + (c0g + c) * 4 + q4];
#pragma unroll
                        for (int c = 0; c < CG; ++c) {
#pragma unroll
                            for (int q4 = 0; q4 < 4; ++q4) {
                                // ACTIVE: the same four fused multiply-adds on scalar registers (measured -1.8 % there and
                                // +0.7 % in the K-pass kernel, same box)
                                if constexpr (MODE == UNERF_FIELD_ACTIVE) {
                                    acc2[c0g + c].x = __builtin_fmaf(dv[4 * q4], wv[c][q4].x, acc2[c0g + c].x);
                                    acc2[c0g + c].y = __builtin_fmaf(dv[4 * q4 + 1], wv[c][q4].y, acc2[c0g + c].y);
                                    acc2[c0g + c].x = __builtin_fmaf(dv[4 * q4 + 2], wv[c][q4].z, acc2[c0g + c].x);
                                    acc2[c0g + c].y = __builtin_fmaf(dv[4 * q4 + 3], wv[c][q4].w, acc2[c0g + c].y);
                                } else {
                                    acc2[c0g + c] = __builtin_elementwise_fma(unerf_v2f{dv[4 * q4], dv[4 * q4 + 1]}, unerf_v2f{wv[c][q4].x, wv[c][q4].y}, acc2[c0g + c]);
                                    acc2[c0g + c] = __builtin_elementwise_fma(unerf_v2f{dv[4 * q4 + 2], dv[4 * q4 + 3]}, unerf_v2f{wv[c][q4].z, wv[c][q4].w}, acc2[c0g + c]);
                                }
                            }
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float half_sum = acc2[c].x + acc2[c].y;
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(half_sum), __float_as_uint(half_sum), false, false);
                    o[c] = (__uint_as_float(sw[0]) + __uint_as_float(sw[1])) + lds[MF_H2_OFF + 192 + c];
                }
            }
            }
            // Epilogue split over the two lane halves (both hold the three colour sums after the exchange; the density
            // logit, row 0, lives in the h = 0 half): h = 0 finishes (density, red), h = 1 (green, blue) -- two
            // exponentials, two reciprocals and two stores per lane instead of four, four and four on half the lanes.
            if (valid) {
                const OutIndex q = out_index(a, k, ts);
                const float x = h ? o[1] : o[0];
                const float y = h ? -o[2] : t[0];                 // h = 1: exp(-blue) for its sigmoid; h = 0: exp(logit)
                // F1 has no lo halves to turn an operand overflow into NaN: an activation beyond 65504 becomes an f16 inf,
                // which reaches every unit of the next layer (inf w, or inf - inf = NaN) and from there the density logit
                // (trunk units) or the three colour sums (head units) -- but sigmoid / exp map +-inf to 0, 1, inf: plausible
                // pixels.  So the four PRE-activation values are tested here (two per lane): two compares per pass.
                if (F1) f1_bad |= !(fabsf(x) < INFINITY) | !(fabsf(y) < INFINITY);
                const float ey = __expf(y);
                const float vy = h ? __builtin_amdgcn_rcpf(1.f + ey) : a.p.average_init_density * ey * sel;
                const float vx = mf_sigmoid_fast(x);
                if (a.p.packed_out) {   // uniform.  (vx, vy) = (red, sigma) in the h = 0 half, (green, blue) in the h = 1 half:
                    // one v_permlane32_swap each brings the upper half's pair down, and the lower half stores 16 bytes
                    // (a column's two lanes are the same sample: `valid` is the same in both)
                    const auto gx = __builtin_amdgcn_permlane32_swap(__float_as_uint(vx), __float_as_uint(vx), false, false);
                    const auto gy = __builtin_amdgcn_permlane32_swap(__float_as_uint(vy), __float_as_uint(vy), false, false);
                    if (h == 0) store_packed(a, k, ts.n, vy, vx, __uint_as_float(gx[1]), __uint_as_float(gy[1]));
                } else {
                    a.rgb[q.rgb + (h ? q.rgb_stride : 0)] = vx;
                    float* py = h ? a.rgb + (q.rgb + 2 * q.rgb_stride) : a.density + q.dens;
                    *py = vy;
                }
                if (MODE == UNERF_FIELD_ACTIVE && h == 0) a.aux[q.aux] = unerf_softplus(t[8]) + a.p.beta_min;
            }
        }
    }
    if (a.p.overflow_flag) {   // one atomic per offending wave and launch
        const uint64_t m = __builtin_amdgcn_ballot_w64(f1_bad);
        if (m != 0 && lane_c == (int)__builtin_ctzll(m)) atomicOr(a.p.overflow_flag, 1);
    }
}
