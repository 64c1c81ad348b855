// The ONE-body tile of gray_stream_kernel (silent_gray.h), a piece of text included in the kernel for the instantiations that are not
// kStreamTwoBodies: every wave, interior or not, runs the general body -- mirror clamps, row and column predicates, padding selects, a
// 64-bit multiply per stored row, the row-program record copied per stream row.  It is the kernel body as it was before
// silent_gray_stream_tile.h, statement for statement, so that these instantiations keep their machine code (registers, waves per SIMD,
// no scratch): K = 8 with 7 levels measured slower with every part of the other text (profiles/r07/README.md), the rest was not measured.
// Reads the kernel's parameters and frame, ty, tx, wave, lane by name.
    constexpr int R = kFusedTH, NR = kStreamRows;
    const FusedLevel& lv = tab.lv[0];  // the one unit level
    const int xw0 = tx * kFusedTW + wave * kFusedCols;
    const bool live = xw0 < lv.out_w;  // wave-uniform: this wave has columns of the level
    const int wx_tile = tx * kFusedWaves + wave;
    const int y0 = ty * R;
    const int ox = xw0 + lane - 4;
    const int W = tab.W;
    frame_src<FT> src;
    if constexpr (kFrameStrided<FT>) src = frame_of(frames, frame);
    else src = frames + (long long)frame * tab.H * W;
    const long long frame_px0 = (long long)frame * tab.frame_px;
    const long long base_px = frame_px0 + lv.px_off;

    // request the 24 frame rows and the per-level column records of this lane (output j of the wave's run = lane j)
    const long long sx = mirror_near(ox, lv.src_w) + lv.src_x0;
    float in[R + 8];
    float in_last = 0.0f, xcol = 0.0f;   // pass 1's sixth taps: stream row R + 8 and the column right of the wave's 64 (unit_taps6)
    constexpr int GR = G < kStreamRegLevels ? G : kStreamRegLevels;
    StreamColT<F64> col[GR > 0 ? GR : 1];
#pragma unroll
    for (int i = 0; i < R + 8; ++i) in[i] = 0.0f;
#pragma unroll
    for (int g = 0; g < GR; ++g) {
        col[g].x0 = col[g].n = col[g].lane4 = 0;
#pragma unroll
        for (int j = 0; j < 6; ++j) col[g].w[j] = 0.0f;
    }
    if (live) {
#pragma unroll
        for (int i = 0; i < R + 8; ++i)
        {
            if constexpr (kFrameStrided<FT>) in[i] = src.at(mirror_near(y0 - 4 + i, lv.src_h) + lv.src_y0, sx);
            else in[i] = (float)src[(long long)(mirror_near(y0 - 4 + i, lv.src_h) + lv.src_y0) * W + sx];
        }
        if constexpr (kFrameStrided<FT>) in_last = src.at(mirror_near(y0 + R + 4, lv.src_h) + lv.src_y0, sx);
        else in_last = (float)src[(long long)(mirror_near(y0 + R + 4, lv.src_h) + lv.src_y0) * W + sx];
        xcol = unit_edge_column(src, W, xw0 + 60, lv.src_w, lv.src_x0, y0 - 4, R + 9, lv.src_h, lv.src_y0, lane);
#pragma unroll
        for (int g = 0; g < GR; ++g) col[g] = stream_col_t<F64>(st, g, wx_tile, lane);
    }
    if (!live) return;
#pragma unroll
    for (int i = 0; i < R + 8; ++i) asm volatile("" ::"v"(in[i]));  // retire loads before the first store
    asm volatile("" : "+v"(in_last), "+v"(xcol));
#pragma unroll
    for (int g = 0; g < GR; ++g) {
        asm volatile("" ::"v"(col[g].lane4));
#pragma unroll
        for (int j = 0; j < 6; ++j) asm volatile("" ::"v"(col[g].w[j]));
    }
#pragma unroll
    for (int i = 0; i < R + 8; ++i) s_rows[wave][i][lane] = in[i];

    // ================= pass 2 (runs first: its registers die before pass 1): every other level of the pyramid,
    // rolled loop over the rows in LDS =================
    acc_t<F64> vacc[G][kStreamSlots];
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int k = 0; k < kStreamSlots; ++k) vacc[g][k] = 0.0f;
    static_assert(G == stream_pad_levels(G), "row programs are padded to 4 or 7 levels");
    constexpr int PR = kStreamProgRow(L, G, F64);
    // constant address space: with a wave-uniform address these are s_load_dwordx16 (no VGPR, no readfirstlane)
    typedef const __attribute__((address_space(4))) int* const_int_ptr;
    const_int_ptr prog = (const_int_ptr)(st.row_prog + (long long)ty * (NR * PR));
    int cur[PR], nxt[PR];
#pragma unroll
    for (int e = 0; e < PR; ++e) cur[e] = prog[e];
    float c0 = s_rows[wave][0][lane];
    const int nr_run = NR;
#pragma unroll 1
    for (int i = 0; i < nr_run; ++i) {
        // record and row of the NEXT step are requested before this step's work
        const int in = min(i + 1, NR - 1);
#pragma unroll
        for (int e = 0; e < PR; ++e) nxt[e] = prog[in * PR + e];
        const float c_next = s_rows[wave][in][lane];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const int meta = cur[g];
            if (!(meta & 128)) continue;  // wave-uniform: this stream row carries no tap of level g
            if constexpr (F64) {
                stream_level_f64<L, G, GR>(g, cur, c0, vacc[g], col, st, wx_tile, lane, pyr, frame_px0, 1, 0);
            } else {
#pragma unroll
                for (int k = 0; k < stream_slots(L, g); ++k) {
                    const float w = __int_as_float(cur[stream_w_off(L, G, g) + k]);
                    const float prev = (meta >> k) & 1 ? 0.0f : vacc[g][k];
                    vacc[g][k] = __builtin_fmaf(w, c0, prev);
                }
                const int done = (meta >> stream_done_shift(L)) & 7;
                if (done != 7) {  // wave-uniform: slot `done` holds a finished output row of level g
                    const int oy = meta >> stream_row_shift(L);
                    float v = vacc[g][0];
#pragma unroll
                    for (int k = 1; k < stream_slots(L, g); ++k) v = done == k ? vacc[g][k] : v;
                    const int vbits = __float_as_int(v);
                    const StreamCol cr = g < GR ? col[g < GR ? g : 0] : stream_col(st, g, wx_tile, lane);   // (g is a constant here)
                    float acc = cr.w[0] * __int_as_float(__builtin_amdgcn_ds_bpermute(cr.lane4, vbits));
#pragma unroll
                    for (int t = 1; t < 6; ++t)
                        acc = __builtin_fmaf(cr.w[t], __int_as_float(__builtin_amdgcn_ds_bpermute(cr.lane4 + 4 * t, vbits)), acc);
                    if (lane < cr.n) pyr[frame_px0 + st.px_off[g] + (long long)oy * st.out_w[g] + cr.x0 + lane] = acc;
                }
            }
        }
#pragma unroll
        for (int e = 0; e < PR; ++e) cur[e] = nxt[e];
        c0 = c_next;
    }

    // ================= pass 1: unit level (pyramid + CS + end), rows back from LDS =================
    // The conv weights live in VGPRs here (K <= 4): a VALU fma whose sources are all VGPRs issues at about twice
    // the rate of one that reads an SGPR once two waves per SIMD are ready (2.7 vs 4.2 cycles per wave
    // instruction, scripts/ubench/valu_rate.hip), and the ~50 SGPRs they would take no longer force reloads of
    // the weights from the kernarg segment in every row.
    constexpr bool VW = K <= 4;
    acc_t<F64> wv[6];
    float csw[9], endw[VW ? 9 * K : 1];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        if constexpr (F64) wv[j] = tab.w64[j];
        else wv[j] = tab.wx[j];  // the unit level's taps are the same on both axes ([1,26,66,26,1]/120 and scipy's sixth, 2^-53)
        if constexpr (VW) asm volatile("" : "+v"(wv[j]));
    }
#pragma unroll
    for (int j = 0; j < 9; ++j) {
        csw[j] = wts.cs[j];
        if constexpr (VW) asm volatile("" : "+v"(csw[j]));
    }
    if constexpr (VW) {
#pragma unroll
        for (int j = 0; j < 9 * K; ++j) {
            endw[j] = wts.end[j];
            asm volatile("" : "+v"(endw[j]));
        }
    }
    const int eff_h = min(lv.zoom_h, lv.out_h), eff_w = min(lv.zoom_w, lv.out_w);
    const bool col_eff = ox >= 0 && ox < eff_w;       // inside the zoomed crop (zero outside it)
    const bool col_in = ox >= 0 && ox < lv.out_w;     // inside the level (zero padding of the convolutions)
    const bool out_lane = lane >= 4 && lane < 4 + kFusedCols && ox < lv.out_w;
    const long long wave_px = base_px + (xw0 - 4);    // + row * out_w + lane: wave-uniform part of every address
    // The two 1-channel maps of the unit level are written with NON-TEMPORAL stores (nt: streamed through L2 without
    // displacing the frame rows that neighbouring tiles re-read): -6...-9 % in alternating A/B.  Measured with it:
    // nt on the 16-byte end-map stores as well +3 %, on those alone 0; nt on the small line-sharing stores of pass 2
    // +18 % (they then reach memory as partial lines); the same nt stores in gray_unit_fused_kernel +6 % (!), in
    // pyramid_unit_kernel and gray_line_end_kernel within noise; a run-time switch between the two kinds of store
    // costs 2.5 % by itself, hence no knob.
    // (Tried and dropped: a 3-instruction relu+clip (v_med3 + NaN select) instead of 4: no measurable change, the kernel
    // is not VALU-bound any more.  Parking 4 finished rows of the 1-channel maps in consumed LDS rows and writing them with one
    // global_store_dwordx4 per 4 rows -- 24 instead of 48 stores per tile -- was 3.5 % slower in an alternating A/B.
    // Round 6, block-wide rows: every wave parks its 56-float pieces of four rows of both maps in consumed LDS rows and, after one
    // barrier per four rows, wave w writes the whole 224-pixel tile row 4 g + w (896 B, 7 whole lines, one 16-byte store per lane).
    // Bit-identical; on the SAME buffers (profiles/r06/evidence/ab_block_rows_same_buffers.txt): config 5 - 8 ... - 13 % on slow
    // placements and + 0.5 ... 1.3 % on fast ones, config 2 + 10 ... 14 % on every placement (the barrier ties four waves that
    // otherwise drift freely).  With the placement tuner choosing the fast relation it only costs: dropped (commit 02244a6 has it).)
    {
        GrayKpAcc ka;
        acc_t<F64> hw[6] = {0, 0, 0, 0, 0, 0};
        float iw[3][3], cw[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) iw[a][b] = cw[a][b] = 0.0f;
#pragma unroll
        for (int i = 0; i < R + 9; ++i) {
            {
                const float c0 = i < R + 8 ? s_rows[wave][i < R + 8 ? i : 0][lane] : in_last;   // (the last row stayed in a register)
                const acc_t<F64> h = unit_taps6(c0, unit_edge(xcol, i), wv);
#pragma unroll
                for (int j = 0; j < 5; ++j) hw[j] = hw[j + 1];
                hw[5] = h;
            }
            if (i >= 5) {
                const int p = y0 + i - 7;
                float v;
                if constexpr (F64) {
                    v = unit_vsum_f64(wv, hw);
                } else {
                    v = wv[0] * hw[0];
#pragma unroll
                    for (int j = 1; j < 6; ++j) v = __builtin_fmaf(wv[j], hw[j], v);
                }
                v = (p >= 0 && p < eff_h && col_eff) ? v : 0.0f;
                if (p >= y0 && p < y0 + R && p < lv.out_h) {  // wave-uniform
                    float* __restrict__ prow = pyr + (wave_px + (long long)p * lv.out_w);
                    if (out_lane) __builtin_nontemporal_store(v, prow + lane);
                }
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    iw[0][b] = iw[1][b];
                    iw[1][b] = iw[2][b];
                }
                iw[2][1] = v;
                iw[2][0] = from_lane_below(v);
                iw[2][2] = from_lane_above(v);
            }
            if (i >= 7) {
                const int c = y0 + i - 8;
                float acc = 0.0f;
                if constexpr (F64) {
                    acc = gray_cs_f64(iw, csw);
                } else {
#pragma unroll
                    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                        for (int dx = 0; dx < 3; ++dx) acc = __builtin_fmaf(iw[dy][dx], csw[dy * 3 + dx], acc);
                }
                // relu (a NaN stays a NaN) and the zero padding of the end convolution in one select
                const float cs = (c >= 0 && c < lv.out_h && col_in && !(acc < 0.0f)) ? acc : 0.0f;
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    cw[0][b] = cw[1][b];
                    cw[1][b] = cw[2][b];
                }
                cw[2][1] = cs;
                cw[2][0] = from_lane_below(cs);
                cw[2][2] = from_lane_above(cs);
            }
            if (i >= 9) {
                const int y = y0 + i - 9;
                if (y < lv.out_h) {  // wave-uniform
                    const long long row_px = wave_px + (long long)y * lv.out_w;
                    if constexpr (kStoreHalf<ST>) {
                        if (cs_out) store_cs_row<true>(cs_out + row_px, cw[1][1], lane, 4, min(kFusedCols, lv.out_w - xw0));
                    } else if (cs_out) {
                        float* __restrict__ crow = cs_out + row_px;
                        if (out_lane) __builtin_nontemporal_store(cw[1][1], crow + lane);
                    }
                    if (end_out) {
                        float acc[K];
                        if constexpr (F64) {
                            gray_end_f64<K>(cw, VW ? endw : wts.end, clip_hi, acc);
                        } else {
#pragma unroll
                            for (int k = 0; k < K; ++k) acc[k] = 0.0f;
#pragma unroll
                            for (int dy = 0; dy < 3; ++dy)
#pragma unroll
                                for (int dx = 0; dx < 3; ++dx)
#pragma unroll
                                    for (int k = 0; k < K; ++k) {
                                        const int wi = (dy * 3 + dx) * K + k;
                                        if constexpr (VW) acc[k] = __builtin_fmaf(cw[dy][dx], endw[wi], acc[k]);
                                        else acc[k] = __builtin_fmaf(cw[dy][dx], wts.end[wi], acc[k]);
                                    }
                            relu_clip_tf(acc, clip_hi);
                        }
                        if constexpr (KP) gray_kp_pixel<K>(kp, acc, y, ox, lv.out_h, lv.out_w, out_lane, kp.value_out + row_px + lane, ka);
                        if constexpr (K == 8) {
                            const int ncols = min(kFusedCols, lv.out_w - xw0);
                            store_row_k8<true>(end_out + row_px * 8, acc, s_slab + wave * 512, lane, 4, ncols);
                        } else if constexpr (kStoreHalf<ST>) {
                            if (out_lane) store_end_px<K, K == 4>(end_out + (row_px + lane) * K, acc);   // (non-temporal where the float32 row is: K = 4)
                        } else if constexpr (K == 4) {
                            // non-temporal like the two 4-byte maps: whole pass -1.6 % (the kernel alone -0.7 %: the rest is
                            // gray_line_end_kernel finding more of the pyramid's levels >= 1 in the Infinity Cache)
                            typedef float nf4 __attribute__((ext_vector_type(4)));
                            nf4* __restrict__ erow = reinterpret_cast<nf4*>(end_out + row_px * 4);
                            if (out_lane) __builtin_nontemporal_store(nf4{acc[0], acc[1], acc[2], acc[3]}, erow + lane);
                        } else {
                            float* __restrict__ po = end_out + row_px * K;
                            if (out_lane) {
#pragma unroll
                                for (int k = 0; k < K; ++k) po[lane * K + k] = acc[k];
                            }
                        }
                    }
                }
                if constexpr (KP) {
                    if (kp_group_ends(i - 9, R)) gray_kp_group_end(kp, ka, frame, kp.level[0], ty, (i - 9) / kSumRows, ox, lv.out_w, out_lane);
                }
            }
        }
        if constexpr (KP) gray_kp_tile_end(kp, ka, frame, kp.level[0], lane);
    }
