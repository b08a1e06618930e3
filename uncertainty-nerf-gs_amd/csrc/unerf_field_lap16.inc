// The LAPLACE split-f16 / single-f16 matrix field kernel.  Included by unerf_nerf.hip (section 5b') TWICE, as two __global__
// templates of one text: UNERF_LAP16_KERNEL = field_kernel_mfma16_laplace (one frame per launch; UNERF_LAP16_VIEWS = false) and
// views_laplace_kernel_mfma16 (XV = LapViews: several views per launch, unerf_field_fwd_laplace_views; UNERF_LAP16_VIEWS =
// true).  Two names, as for unerf_field_mfma16.inc: the single-view kernels stay the kernels they were, and the set of
// field_kernel* instantiations stays what field_launch() can launch.
template <int TCNN, bool F1 = false, typename... XV>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((F1 && !TCNN) ? 3 : 2))) void UNERF_LAP16_KERNEL(FieldArgs a, uint32_t num_tiles, FastDiv div_s, XV... xv) {
    constexpr bool VW = xv_is_lap_views<XV...>::value;   // XV = LapViews: ray blocks laid out per view, a sample-set base per view
    static_assert(VW || sizeof...(XV) == 0, "trailing argument: LapViews or none");
    static_assert(VW == UNERF_LAP16_VIEWS, "LapViews rides on views_laplace_kernel_mfma16, and nothing else does");
    extern __shared__ float lds[];
    const int32_t* vsets = nullptr;
    if constexpr (VW) {   // the per-view table goes through LDS: a by-value array under a run-time index would go to scratch
        __shared__ int32_t s_vset[UNERF_NERF_MAX_VIEWS];
        if (threadIdx.x < UNERF_NERF_MAX_VIEWS) s_vset[threadIdx.x] = lv_of(xv...).set_base[threadIdx.x];
        vsets = s_vset;
    }
    {
        const float4* src = reinterpret_cast<const float4*>(a.p.mfma16_blob);
        float4* dst = reinterpret_cast<float4*>(lds);
        for (int i = threadIdx.x; i < UNERF_MFMA_BLOB_FLOATS / 4; i += 256) dst[i] = src[i];
    }
    __shared__ uint32_t s_tl[TCNN ? MF_TL_WORDS : 1];
    // The bias rows of the sampled heads (16 per lane half and row block: the accumulators' initial values).  As global
    // loads in front of every block's first MFMA they were the one load of the head loop whose latency nothing hid --
    // 16 round trips to L2 per tile.  Each wave brings its tile's 512 words in with two 16-byte loads per lane while the
    // hash grid is gathered, parks them in LDS, and the blocks read them back with ds_read_b128.
    __shared__ float s_lbias[4][512];
    if (TCNN) mf_stage_tcnn_levels<(TCNN == 2 ? 2 : 3)>(a, s_tl);
    __syncthreads();
    const int lane_c = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane_c & 31, h = lane_c >> 5;
    const uint32_t mask = (1u << a.p.log2T) - 1u;
    const float inv_n = 1.f / (float)a.p.n_lap, inv_nr = 1.f / (float)a.p.n_lap_rgb;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, bpx = gridDim.x >> 3;
    const uint32_t tpx = (num_tiles + 7u) / 8u;
    const uint32_t tile_end = (xcd + 1) * tpx < num_tiles ? (xcd + 1) * tpx : num_tiles;
    bool f1_bad = false;   // F1: a sampled-head mean of this lane came out inf / NaN
    for (uint32_t tile = xcd * tpx + (uint32_t)slot * 4u + (uint32_t)wv; tile < tile_end; tile += (uint32_t)bpx * 4u) {
        int lane = lane_c;
        asm volatile("" : "+v"(lane));
        TileSample ts;
        if constexpr (VW) ts = tile_sample_views(a, tile, div_s, j, lv_of(xv...));
        else ts = tile_sample(a, tile, div_s, j);
        // the blob of the tile's sample set (wave-uniform: scalar arithmetic in both forms)
        auto set_blob = [&](const float* blob) -> const float* {
            if constexpr (VW) return lap_set_blob_views(a, blob, tile, div_s, lv_of(xv...), vsets);
            else return lap_set_blob(a, blob, tile, div_s);
        };
        const bool valid = ts.valid;
        const int64_t n = ts.n;
        const float dxr = ts.dx, dyr = ts.dy, dzr = ts.dz;
        float px = ts.px, py = ts.py, pz = ts.pz;
        // inference: the returned mu_d is NOT selector-masked (laplace_field.py:356-362) unless lap_mask_density
        const float sel = unerf_normalize_position(px, py, pz, a.box);
        constexpr bool BIAS_LDS = !(F1 && !TCNN);
        float4 lb0, lb1;
        if (BIAS_LDS) {
            const float4* lbsrc = reinterpret_cast<const float4*>(set_blob(a.p.lap16_blob) + LAP_BIAS_OFF) + lane_c * 2;
            lb0 = lbsrc[0];
            lb1 = lbsrc[1];
        }
        u32x8 feat_pk;
        const f32x16 feat = mf_gather_feats<true, TCNN>(a, px, py, pz, h, mask, s_tl, &feat_pk);
        if (BIAS_LDS) {   // (the previous tile's heads are done with the buffer: a wave's LDS operations execute in order)
            float4* dst = reinterpret_cast<float4*>(s_lbias[wv]) + lane_c * 2;
            dst[0] = lb0;
            dst[1] = lb1;
        }

        const float* lap16 = set_blob(a.p.lap16_blob);
        // (the single-product kernel at three waves per SIMD has no registers for a third operand buffer: it keeps the
        // one-block-ahead heads)
        constexpr bool STREAM = !(F1 && !TCNN);
        // base_mlp: bare Linear 32 -> 64 (no ReLU, utils.py:22-23)
        f32x16 hb0 = mf16_bias(lds, 0, h), hb1 = mf16_bias(lds, 1, h);
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            f16x8 bhi, blo;
            mf16_feat_operand<TCNN, F1>(feat, feat_pk, st, bhi, blo);
            mf16_mac2<F1, TCNN == 2>(lds, 2 * st, 2 * st + 1, lane, bhi, blo, hb0, hb1);
        }
        // the 64 base outputs feed both mlp_hidden (geo) and the sampled density rows: split them once
        f16x8 xhi[4], xlo[4];
#pragma unroll
        for (int st = 0; st < 4; ++st) mf16_split<F1>(st < 2 ? hb0 : hb1, st & 1, xhi[st], xlo[st]);
        f32x16 t = mf16_bias(lds, 2, h);
#pragma unroll
        for (int st = 0; st < 4; ++st) t = mf16_mac<F1>(lds, 4 + st, lane, xhi[st], xlo[st], t);
        float d1, d2;
        if constexpr (STREAM) {
            float ds1[1], ds2[1];
            if (a.p.lap_softplus) mf16_lap_stream<2, F1, 1>(lap16, s_lbias[wv], 0, a.p.n_lap, lane, xhi, xlo, h, ds1, ds2);   // uniform
            else mf16_lap_stream<0, F1, 1>(lap16, s_lbias[wv], 0, a.p.n_lap, lane, xhi, xlo, h, ds1, ds2);
            d1 = ds1[0];
            d2 = ds2[0];
        } else {
            if (a.p.lap_softplus) mf16_lap_head<2, F1>(lap16, 0, a.p.n_lap, lane, xhi, xlo, h, d1, d2);   // uniform
            else mf16_lap_head<0, F1>(lap16, 0, a.p.n_lap, lane, xhi, xlo, h, d1, d2);
        }
        float mu_d = d1 * inv_n, mu2_d = d2 * inv_n;
        if (a.p.lap_mask_density) {  // use_deterministic_density: selector-masked mean, no variance
            mu_d *= sel;
            mu2_d = mu_d * mu_d;
        }

        // colour trunk: [geo15 | SH16] -> 64 -> 64
        f32x16 c0 = mf16_bias(lds, 3, h), c1 = mf16_bias(lds, 4, h);
        {
            f16x8 bhi, blo;
            mf16_split<F1>(t, 0, bhi, blo);
            mf16_mac2<F1>(lds, 8, 9, lane, bhi, blo, c0, c1);
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
            mf16_split8<F1>(mine, bhi, blo);
            mf16_mac2<F1>(lds, 10, 11, lane, bhi, blo, c0, c1);
        }
        // (an overflowed operand of the split form makes every unit of the next layer NaN, which the integer-maximum ReLU
        // may turn into 0: one accumulator per colour layer is tested first -- see field_kernel_mfma16)
        if (!F1) f1_bad |= c0[0] != c0[0];
        c0 = mf_relu(c0);
        c1 = mf_relu(c1);
        f32x16 x0 = mf16_bias(lds, 5, h), x1 = mf16_bias(lds, 6, h);
        mf16_layer64<2, F1>(lds, 12, lane, c0, c1, x0, x1);
        if (!F1) f1_bad |= x0[0] != x0[0];
        x0 = mf_relu(x0);
        x1 = mf_relu(x1);
#pragma unroll
        for (int st = 0; st < 4; ++st) mf16_split<F1>(st < 2 ? x0 : x1, st & 1, xhi[st], xlo[st]);
        float mu_c[3], vsum = 0.f;
        if constexpr (STREAM) {
            float cs1[3], cs2[3];
            mf16_lap_stream<1, F1, 3>(lap16, s_lbias[wv], 1, a.p.n_lap_rgb, lane, xhi, xlo, h, cs1, cs2);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                mu_c[c] = cs1[c] * inv_nr;
                vsum += fmaxf(cs2[c] * inv_nr - mu_c[c] * mu_c[c], 0.f);
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float c1s, c2s;
                mf16_lap_head<1, F1>(lap16, 1 + c, a.p.n_lap_rgb, lane, xhi, xlo, h, c1s, c2s);
                mu_c[c] = c1s * inv_nr;
                vsum += fmaxf(c2s * inv_nr - mu_c[c] * mu_c[c], 0.f);
            }
        }
        // F1: an f16 operand beyond 65504 turns the sampled rows into +-inf / NaN; a density mean of +inf from a FINITE
        // logit is not possible below e^88, so non-finite means are treated as operand overflow (see field_kernel_mfma16)
        if (F1 && valid) f1_bad |= !(fabsf(mu_d) < INFINITY) | !(fabsf(mu_c[0] + mu_c[1] + mu_c[2]) < INFINITY);
        if (valid && h == 0) {
            a.density[n] = mu_d;
            a.aux[n] = mu2_d - mu_d * mu_d;
            a.aux2[n] = vsum / 3.f;
            a.rgb[n * 3 + 0] = mu_c[0];
            a.rgb[n * 3 + 1] = mu_c[1];
            a.rgb[n * 3 + 2] = mu_c[2];
        }
    }
    if (a.p.overflow_flag) {
        const uint64_t m = __builtin_amdgcn_ballot_w64(f1_bad);
        if (m != 0 && lane_c == (int)__builtin_ctzll(m)) atomicOr(a.p.overflow_flag, 1);
    }
}
