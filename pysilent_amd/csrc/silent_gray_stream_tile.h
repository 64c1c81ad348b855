// The tile body of the kStreamTwoBodies instantiations of gray_stream_kernel (silent_gray.h): everything a wave does once block and
// wave are known.  Not a header of its own but the text of gray_stream_tile<INTERIOR>; it reads that function's parameters and template
// parameters by name.  (The other instantiations: silent_gray_stream_tile_general.h.)
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
    float in[R + 8];
    float in_last = 0.0f, xcol = 0.0f;   // pass 1's sixth taps: stream row R + 8 and the column right of the wave's 64 (unit_taps6)
    constexpr int GR = G < kStreamRegLevels ? G : kStreamRegLevels;
    StreamColT<F64> col[GR > 0 ? GR : 1];
    if constexpr (INTERIOR) {
        // one wave-uniform row cursor, advanced by the row stride; the lane's column is the per-lane offset of every load
        const int sy0 = y0 - 4 + lv.src_y0, sx0 = xw0 - 4 + lv.src_x0;
        if constexpr (kFrameStrided<FT>) {
            auto row = src;
            global_ptr<const unsigned char> rp = (global_ptr<const unsigned char>)(src.p + (sy0 * src.row_stride + sx0 * src.pixel_stride));
#pragma unroll
            for (int i = 0; i < R + 9; ++i) {
                row.p = (const unsigned char*)rp;
                const float f = row.at(0, lane);
                if (i < R + 8) in[i < R + 8 ? i : 0] = f;
                else in_last = f;
                advance_rows(rp, src.row_stride);
            }
            xcol = src.at(sy0 + min(lane, R + 8), sx0 + 64);
        } else {
            global_ptr<const FT> rp = (global_ptr<const FT>)(src + ((long long)sy0 * W + sx0));
#pragma unroll
            for (int i = 0; i < R + 9; ++i) {
                const float f = (float)((const FT*)rp)[lane];
                if (i < R + 8) in[i < R + 8 ? i : 0] = f;
                else in_last = f;
                advance_rows(rp, W);
            }
            xcol = (float)src[(long long)(sy0 + min(lane, R + 8)) * W + (sx0 + 64)];
        }
#pragma unroll
        for (int g = 0; g < GR; ++g) col[g] = stream_col_t<F64>(st, g, wx_tile, lane);
    } else {
        const long long sx = mirror_near(ox, lv.src_w) + lv.src_x0;
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
    }
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
    // Two stream rows per iteration, the two records swapping roles (h = 0: rec[0] is this row's, rec[1] receives the next one;
    // h = 1 the other way round), so no record is copied.  Record and row of the NEXT step are requested before this step's work.
    static_assert(NR % 2 == 0, "pass 2 runs two stream rows per iteration");
    constexpr int HS = 2;
    int rec[2][PR];
    float cv[2];
#pragma unroll
    for (int e = 0; e < PR; ++e) rec[0][e] = prog[e];
    cv[0] = s_rows[wave][0][lane];
#pragma unroll 1
    for (int i = 0; i < NR; i += HS) {
#pragma unroll
        for (int h = 0; h < HS; ++h) {
            const int (&cur)[PR] = rec[h];
            const float c0 = cv[h];
            const int in = min(i + h + 1, NR - 1);
#pragma unroll
            for (int e = 0; e < PR; ++e) rec[h ^ 1][e] = prog[in * PR + e];
            cv[h ^ 1] = s_rows[wave][in][lane];
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
        }
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
    const bool col_eff = INTERIOR || (ox >= 0 && ox < eff_w);       // inside the zoomed crop (zero outside it)
    const bool col_in = INTERIOR || (ox >= 0 && ox < lv.out_w);     // inside the level (zero padding of the convolutions)
    const bool out_lane = lane >= 4 && lane < 4 + kFusedCols && (INTERIOR || ox < lv.out_w);
    const long long wave_px = base_px + (xw0 - 4);    // + row * out_w + lane: wave-uniform part of every address
    // One wave-uniform pointer per output stream at lane 0 of the tile's first row, advanced by one row of the level per row step
    // (advance_rows: an addition in SGPRs).  A store then takes this scalar base and the lane's 32-bit byte offset.
    // (cs_out / end_out may be null -- a map that was not asked for: its pointer is formed and advanced all the same and never
    // dereferenced, every store below stands under `if (cs_out)` / `if (end_out)`.)
    global_ptr<float> prow = (global_ptr<float>)(pyr + (wave_px + (long long)y0 * lv.out_w));
    global_ptr<ST> crow = (global_ptr<ST>)(cs_out + (wave_px + (long long)y0 * lv.out_w));
    global_ptr<ST> erow = (global_ptr<ST>)(end_out + (wave_px + (long long)y0 * lv.out_w) * K);
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
    // Round 7, the scalar side (profiles/r07/README.md; the kernel issued as many scalar as vector instructions, about 2000 each per
    // wave): the INTERIOR body, the row pointers and pass 2 without its record copy took the config-2 kernel from 0.783 to 0.74 -
    // 0.76 ms on the same buffers, each step a gain of its own.  Tried with them and dropped: ONE exec region per row step around its
    // up to three per-lane stores (the row conditions inside it; 52 -> 22 saveexec per body): + 1 % on two of three allocations on
    // config 2, + 1.5 % on config 5 -- the stores then all wait for the end of the row step.
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
                if constexpr (!INTERIOR) v = (p >= 0 && p < eff_h && col_eff) ? v : 0.0f;
                if (p >= y0 && p < y0 + R && (INTERIOR || p < lv.out_h)) {  // wave-uniform
                    if (out_lane) __builtin_nontemporal_store(v, (float*)prow + lane);
                    advance_rows(prow, lv.out_w);
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
                const float cs = (INTERIOR || (c >= 0 && c < lv.out_h && col_in)) && !(acc < 0.0f) ? acc : 0.0f;
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
                if (INTERIOR || y < lv.out_h) {  // wave-uniform
                    ST* __restrict__ crow_y = (ST*)crow;
                    ST* __restrict__ erow_y = (ST*)erow;
                    if constexpr (kStoreHalf<ST>) {
                        if (cs_out) store_cs_row<true>(crow_y, cw[1][1], lane, 4, INTERIOR ? kFusedCols : min(kFusedCols, lv.out_w - xw0));
                    } else if (cs_out) {
                        if (out_lane) __builtin_nontemporal_store(cw[1][1], crow_y + lane);
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
                        if constexpr (KP) gray_kp_pixel<K>(kp, acc, y, ox, lv.out_h, lv.out_w, out_lane, kp.value_out + (wave_px + (long long)y * lv.out_w) + lane, ka);
                        if constexpr (K == 8) {
                            const int ncols = INTERIOR ? kFusedCols : min(kFusedCols, lv.out_w - xw0);
                            store_row_k8<true>(erow_y, acc, s_slab + wave * 512, lane, 4, ncols);
                        } else {
                            if (out_lane) store_end_lane<K>(erow_y, lane, acc);
                        }
                    }
                    advance_rows(crow, lv.out_w);
                    advance_rows(erow, (long long)lv.out_w * K);
                }
                if constexpr (KP) {
                    if (kp_group_ends(i - 9, R)) gray_kp_group_end(kp, ka, frame, kp.level[0], ty, (i - 9) / kSumRows, ox, lv.out_w, out_lane);
                }
            }
        }
        if constexpr (KP) gray_kp_tile_end(kp, ka, frame, kp.level[0], lane);
    }
