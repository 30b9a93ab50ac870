// (Not a header: the body of two kernels, included inside their definitions -- see below.  Named .h so that the
// hash of the kernel sources, bench.kernel_sources_sha, covers it.)
// Body of the block-encode kernels k_screen_encode<PROBE, MODE> and k_gray_encode<PROBE> (MODE 3), included inside
// each kernel's definition (jpeg_screen_kernels.hip).  An include, not a __forceinline__ device function: the inliner
// optimises a callee on its own before it inlines it, which changed the code of the existing forms (other register
// assignment, other load order); included, the existing forms compile to the same instructions as before the gray
// form existed.  In scope: the kernel parameters g, n_frames, rgb (the input bytes), sp and the template parameters
// PROBE, MODE.
    constexpr bool STD = MODE != 0, S420 = MODE == 2, GRAY = MODE == 3;
    constexpr uint32_t kPasses = S420 ? 6u : (GRAY ? 1u : 3u);
    // Standard 4:4:4 converts whole tiles on the matrix units (jpeg_screen_devfn.h: +4 %).  4:2:0 does not: the same
    // scheme for its chroma passes was built and measured at -1.5 % (profiles/r03_f_*) -- a matrix
    // instruction costs the issuing wave what 2.5 plain VALU instructions cost, the fixed-point form needs only four of
    // those per pixel, and the fragments' registers push the kernel to the limit beyond which the tail kernels stop
    // running beside it.
    constexpr bool kCscMfma = MODE == 1;
    // Strict mode forms the reference's integer numerators on the matrix units too (strict_rowpair_mfma); division, luma's
    // remainder test and the chroma means stay on the vector units.  Bit-exact either way; which is faster depends on the
    // instruction scheduling: under the backend's default strategy the matrix form lost 9 % (gpurun r4cu: its results arrive
    // late in a phase with nothing else to issue), under iterative-ilp it wins 1.2 % (269.8 against 266.5, gpurun r4cs2).
    constexpr bool kCscMfmaStrict = MODE == 0;
    __shared__ uint32_t s_tbuf_all[kEncWaves][kRowWords];          // zig-zag rows, int16 [position][unit] (jpeg_screen_devfn.h)
    __shared__ alignas(16) uint32_t s_slot_all[kEncWaves][(kSlotRows + 1) * 64];  // AC strings [word][lane] + dump row
    __shared__ uint32_t s_mask_all[kEncWaves][2][64];              // non-zero masks (lo, hi)
    __shared__ float s_qf[2][16][8];    // per group of 4 positions: 2^-23/Q x4 (first look: top three digits), its thresholds x4
    __shared__ uint32_t s_act[2][256];  // (run,size) AC tables
    __shared__ uint32_t s_lut2[2][kLut2Words];  // (value,run) symbol tables
    __shared__ uint32_t s_dc[2][16];      // DC tables

    const uint32_t tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, n = lane & 15, gq = lane >> 4;
    uint32_t* s_tbuf = s_tbuf_all[wv];
    uint32_t* s_slot = s_slot_all[wv];
    uint32_t* s_mlo = s_mask_all[wv][0];
    uint32_t* s_mhi = s_mask_all[wv][1];
    for (uint32_t i = tid; i < 512; i += 256) {
        (&s_act[0][0])[i] = sp.lut[512 + i];
    }
    for (uint32_t i = tid; i < 2 * kLut2Words; i += 256) (&s_lut2[0][0])[i] = sp.lut2[i];
    (&s_qf[0][0][0])[tid] = sp.qconst_f[tid];
    if (tid < 32) s_dc[tid >> 4][tid & 15] = sp.lut[(tid >> 4) * 256 + (tid & 15)];
    if (lane < 32) s_tbuf[64 * 32 + lane] = kRowSentinel * 0x00010001u;  // sentinel row after zig-zag position 63 (never written again)
    i16a* const tb16 = reinterpret_cast<i16a*>(s_tbuf);
    // A fragments of the top three digits stay in registers; the two low digits only matter for the
    // (rare) second look and are fetched on demand.
    v4i A[4][kLookDigits];
    load_look_fragments(sp, lane, A);
    // quantiser divisors of coefficient 0, read once: a load per pass would sit behind everything the wave has in flight
    // (vmcnt retires in issue order), the next pass's first rows included
    const double q0_luma = sp.qd[0], q0_chroma = sp.qd[64];
    __syncthreads();

    // Work distribution.  With a grid that is a multiple of 8 workgroups, the waves of XCD x
    // (workgroups x, x+8, ...) take the tiles congruent to x mod 8, channel by channel, so
    // that the three channels of a tile are processed side by side in one XCD and share its
    // RGB bytes in that L2.  Speed only: any mapping is correct.
    const uint32_t gwave = blockIdx.x * kEncWaves + wv;   // global wave id
    const uint32_t per_frame = g.tiles * kPasses;
    const bool xcd_map = (gridDim.x % 8u) == 0u;
    const uint32_t xcd = blockIdx.x % 8u;
    const uint32_t local = (blockIdx.x / 8u) * kEncWaves + wv;       // index of this wave inside its XCD
    const uint32_t local_n = (gridDim.x / 8u) * kEncWaves;           // waves per XCD
    const uint32_t tiles_x = xcd_map ? (g.tiles + 7u - xcd) / 8u : 0u;  // tiles this XCD owns per frame
    const uint32_t pairs_total = xcd_map ? tiles_x * kPasses * n_frames : per_frame * n_frames;
    const uint32_t pstart = xcd_map ? local : gwave;
    const uint32_t pstep = xcd_map ? local_n : gridDim.x * kEncWaves;

    // Stagger (MI355X_MICROARCH.md, two waves per SIMD, item 9): the two workgroups of a CU otherwise run in lockstep --
    // both waves of a SIMD in the issue-heavy transform, then both in the latency-bound walk.  Starting the
    // later-dispatched workgroup about half a pass late puts one wave's walk beside the other's transform.
    if (blockIdx.x >= sp.prio_from_wg)
        for (uint32_t i = 0; i < sp.stagger; ++i) __builtin_amdgcn_s_sleep(127);
    WaveArena wa{gwave * sp.region_words, sp.region_words};
#ifdef MI355_STAMPS
    unsigned long long stamp_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, stamp_prev, wave_t0, wave_t1;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(wave_t0)::"memory");  // 100 MHz wall clock
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_prev)::"memory");
#endif
    bool walk_general[2] = {false, false};  // per channel type: the last pass had a symbol-table miss (walk_nonzeros)
    uint32_t n_rewalked = 0, n_general = 0;  // mi355_jpeg_screen_stats: summed per wave, added once at the end (one
                                             // atomic per pass on one address would serialise the whole device at q90)
    // One pass = one (frame, tile, pass) of this wave's share.  Its coordinates are worked out one pass AHEAD, and the
    // first row pair of the next pass is requested before the entropy walk of the current one: the load (an HBM miss for
    // the first of a tile's three channel waves) lands during the walk instead of stalling the next pass at its first
    // instruction, and because vmcnt retires in issue order it does not wait behind this pass's scattered string stores.
    struct Pass {
        uint32_t frame, tile, chan;
        // block (or MCU) coordinates of this lane's four units: x | y << 16 (packed: registers).  Four scalars, not an
        // array: an array member kept the struct in memory (the optimiser's 20-byte alloca was then promoted to LDS --
        // 5 KB per workgroup, enough to push the tail kernels off the CU: -25 % on batches)
        uint32_t b0, b1, b2, b3;
        bool fast;
        __device__ __forceinline__ uint32_t bxy(int j) const { return j == 0 ? b0 : (j == 1 ? b1 : (j == 2 ? b2 : b3)); }
        __device__ __forceinline__ void set_bxy(int j, uint32_t v) {
            if (j == 0) b0 = v;
            else if (j == 1) b1 = v;
            else if (j == 2) b2 = v;
            else b3 = v;
        }
    };
    auto locate = [&](uint32_t p) -> Pass {
        Pass ps;
        uint32_t frame, tile, chan;
        if (xcd_map) {
            const uint32_t pf = tiles_x * kPasses;
            frame = p / pf;
            const uint32_t q = p - frame * pf;
            tile = (q / kPasses) * 8u + xcd;
            chan = q % kPasses;
        } else {
            frame = p / per_frame;
            const uint32_t q = p - frame * per_frame;
            tile = q / kPasses;
            chan = q % kPasses;
        }
        const bool luma420 = S420 && chan < 4u;

        // block coordinates of this lane's four blocks (16j + n), and whether the whole tile
        // lies inside the image (no mirror padding)
        bool interior = true;
        if constexpr (S420) {
            // MCU of this lane's unit in sub-tile j: luma pass s: 16 s + 4 j + n / 4 (block k = n & 3 of it),
            // chroma pass: 16 j + n.  For chroma passes bxy holds MCU coordinates.
            const uint32_t step = luma420 ? 4u : 16u;
            uint32_t m = tile * 64 + (luma420 ? 16 * chan + (n >> 2) : n);
            uint32_t my = m / g.nmx, mx = m - my * g.nmx;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (m >= g.N) {  // past the last MCU: any valid one will do, the lane is masked later
                    mx = g.nmx - 1;
                    my = g.N / g.nmx - 1;
                }
                if (luma420) {
                    const uint32_t lx = 2 * mx + (n & 1), ly = 2 * my + ((n >> 1) & 1);
                    ps.set_bxy(j, lx | (ly << 16));
                    interior = interior && (lx * 8 + 8 <= g.W) && (ly * 8 + 8 <= g.H);
                } else {
                    ps.set_bxy(j, mx | (my << 16));
                    interior = interior && (mx * 16 + 16 <= g.W) && (my * 16 + 16 <= g.H);
                }
                m += step;
                mx += step;
                while (mx >= g.nmx) {
                    mx -= g.nmx;
                    ++my;
                }
            }
        } else {
            uint32_t b = tile * 64 + n;
            uint32_t by = b / g.nbx, bx = b - by * g.nbx;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t bb = tile * 64 + 16 * j + n;
                if (bb >= g.N) {  // past the last block: any valid block will do, the lane is masked later
                    bx = g.nbx - 1;
                    by = g.N / g.nbx - 1;
                }
                ps.set_bxy(j, bx | (by << 16));
                interior = interior && (bx * 8 + 8 <= g.W) && (by * 8 + 8 <= g.H);
                bx += 16;
                while (bx >= g.nbx) {
                    bx -= g.nbx;
                    ++by;
                }
            }
        }
        ps.fast = g.fast_rows && !wave_any(!interior);
        ps.frame = frame, ps.tile = tile, ps.chan = chan;
        return ps;
    };
    uint32_t raw[12];  // raw RGB of the row pair to convert next (fast path)
    uint32_t graw[4];  // gray: the next row pair's 16 samples
    RawChunk Xn[4];    // the same for the matrix-unit conversion (standard 4:4:4): the next row pair's four chunks
    v4i F[4];          // ... and the colour-conversion fragments of the pass they belong to
    auto request_first_rows = [&](const Pass& ps) {
        const bool chroma420 = S420 && ps.chan >= 4u;
        if (!ps.fast) return;
        const uint8_t* pf = rgb + (size_t)ps.frame * g.frame_stride;
        if constexpr (GRAY) {
            load_gray_rowpair(pf, g, ps.b0 & 0xffffu, ps.b0 >> 16, gq, graw);
        } else if constexpr (kCscMfma) {
            // the pass's colour-conversion fragments travel with its first rows: requested before the walk of the pass in
            // front, they do not queue behind that pass's string stores (vmcnt retires in issue order)
            load_csc_fragments(sp, lane, (int)ps.chan * 4, F);
            load_std_rowpair(pf, g, ps.b0 & 0xffffu, ps.b0 >> 16, gq, Xn);
        } else {
            if constexpr (kCscMfmaStrict) {  // the pass's two digit sets (F[0], F[1]) travel with its first rows
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const uint4 t = sp.csc_frag[(kCscSets + (int)ps.chan * 2 + i) * 64 + lane];
                    F[i] = v4i{(int)t.x, (int)t.y, (int)t.z, (int)t.w};
                }
            }
            if (!chroma420) load_raw_rowpair(pf, g, ps.b0 & 0xffffu, ps.b0 >> 16, gq, raw);
        }
    };
    Pass cur{}, nxt{};
    if (pstart < pairs_total) {
        cur = locate(pstart);
        request_first_rows(cur);
    }
    for (uint32_t p = pstart; p < pairs_total; p += pstep) {
        STAMP(7);
        const uint32_t frame = cur.frame, tile = cur.tile, chan = cur.chan;
        // `chan` is the pass; the colour component differs from it only in 4:2:0 (passes 0..3 = luma)
        const uint32_t comp = S420 ? (chan < 4u ? 0u : chan - 3u) : chan;
        const bool luma420 = S420 && chan < 4u, chroma420 = S420 && chan >= 4u;
        const uint32_t ct = comp ? 1u : 0u;
        const uint8_t* f = rgb + (size_t)frame * g.frame_stride;
        const bool avg = !STD && (comp != 0) && (g.flags & 1u);  // standard mode never replicates chroma means
        const size_t us_base = (((size_t)frame * g.tiles + tile) * kPasses + chan) * 64;
        const bool fast = cur.fast;

        STAMP(0);
        // Issue arbitration is oldest-first, and the two workgroups of a CU are dispatched in grid
        // order: without help the waves of the later-dispatched half of the grid get the leftover
        // issue slots and finish ~20 % later than the others (measured with in-kernel timestamps:
        // mean wave end 41.5 vs 49.3 us), leaving the SIMDs half empty at the end.  Raising their
        // priority outside the (LDS-latency-bound) entropy walk equalises the two halves
        // (45.9 vs 45.4 us) and shortens the kernel by 8 %.  Only when this launch fills the device with
        // exactly two workgroups per CU (sp.prio_from_wg = number of CUs, else none): half-device launches
        // of pipelined callers share each CU with another stream's kernel and do better without it (+3 %).
        // Speed only.
        if (blockIdx.x >= sp.prio_from_wg) __builtin_amdgcn_s_setprio(1);

        s_mlo[lane] = 0;
        s_mhi[lane] = 0;
        __builtin_amdgcn_wave_barrier();

        const bool on_mfma = kCscMfma && fast;
        // raw RGB of unit-tile j+1 is fetched while unit-tile j is processed (that of unit-tile 0 was requested a pass ago)
        uint32_t dcsum = 0;  // sample sum of the block whose coefficient 0 this lane will form
        // scale factors and accept thresholds of the NEXT quantiser group, requested one group ahead (see the loop below)
        v4f qf_s = *reinterpret_cast<const v4f*>(&s_qf[ct][gq][0]), qf_h = *reinterpret_cast<const v4f*>(&s_qf[ct][gq][4]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t bx = cur.bxy(j) & 0xffffu, by = cur.bxy(j) >> 16;
            uint32_t pk[4];  // 16 samples; on_mfma: as sample - 128 (int8), else unsigned
            if (on_mfma) {
                if constexpr (kCscMfma) {
                    // (one buffer: the next row pair lands during the quantiser)
                    if (comp) std_rowpair_mfma<true>(Xn, F, pk);
                    else std_rowpair_mfma<false>(Xn, F, pk);
                    if (j < 3) load_std_rowpair(f, g, cur.bxy(j + 1) & 0xffffu, cur.bxy(j + 1) >> 16, gq, Xn);
                }
            } else if (GRAY) {
                if constexpr (GRAY) {  // the samples as they are: no colour conversion
                    if (fast) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) pk[i] = graw[i];
                        if (j < 3) load_gray_rowpair(f, g, cur.bxy(j + 1) & 0xffffu, cur.bxy(j + 1) >> 16, gq, graw);
                    } else {
                        generic_gray_rowpair(f, g, bx, by, gq, pk);
                    }
                }
            } else if (chroma420) {
                if constexpr (S420) {  // rows 2gq, 2gq+1 of the MCU's 8x8 chroma block <- pixel rows 4gq .. 4gq+3
                    if (fast) {
#pragma unroll 1
                        for (uint32_t half = 0; half < 2; ++half) {  // one chroma row at a time: 24 live dwords
                            uint32_t w24[24], o[2];
                            load_raw_mcu_rows(f, g, bx, by, 4 * gq + 2 * half, w24);
                            if (comp == 1) convert_chroma420_row<1>(w24, o);
                            else convert_chroma420_row<2>(w24, o);
                            if (half == 0) pk[0] = o[0], pk[1] = o[1];
                            else pk[2] = o[0], pk[3] = o[1];
                        }
                    } else {
                        generic_chroma420(f, g, (int)comp, bx, by, gq, pk);
                    }
                }
            } else if (fast) {
                uint32_t rp[12];
#pragma unroll
                for (int i = 0; i < 12; ++i) rp[i] = raw[i];
                if (j < 3) load_raw_rowpair(f, g, cur.bxy(j + 1) & 0xffffu, cur.bxy(j + 1) >> 16, gq, raw);  // (two pairs in flight: -1 %)
                if constexpr (kCscMfmaStrict) {
                    const v4i (&F2)[2] = reinterpret_cast<const v4i (&)[2]>(F);
                    if (comp == 0) strict_rowpair_mfma<0>(rp, F2, splat4(kCscStrictC[0]), false, pk);
                    else strict_rowpair_mfma<1>(rp, F2, splat4(kCscStrictC[1]), avg, pk);  // (the fragments say which chroma channel)
                } else {
                    if (comp == 0) convert_rowpair<0, STD>(rp, false, pk);
                    else if (comp == 1) convert_rowpair<1, STD>(rp, avg, pk);
                    else convert_rowpair<2, STD>(rp, avg, pk);
                }
            } else {
                if (comp == 0) generic_rowpair<0, STD>(f, g, false, bx, by, gq, pk);
                else if (comp == 1) generic_rowpair<1, STD>(f, g, avg, bx, by, gq, pk);
                else generic_rowpair<2, STD>(f, g, avg, bx, by, gq, pk);
            }
            if constexpr (PROBE && !S420) {
                if (sp.samples && tile * 64 + 16 * j + n < g.N) {
#pragma unroll
                    for (int sidx = 0; sidx < 16; ++sidx) {
                        uint32_t v = ((pk[sidx >> 2] ^ (on_mfma ? 0x80808080u : 0u)) >> (8 * (sidx & 3))) & 255u;
                        size_t px = (size_t)(by * 8 + gq * 2 + (sidx >> 3)) * g.W8 + bx * 8 + (sidx & 7);
                        sp.samples[((size_t)frame * g.W8 * g.H8 + px) * (GRAY ? 1 : 3) + chan] = (uint8_t)v;
                    }
                }
            }
            STAMP(5);
            // sum of the block's 64 samples (for the exact DC): 16 in this lane, then over the 4 row-pair lanes
            uint32_t ssum = 0;
            v4i B;
            if (on_mfma) {  // signed bytes already: the sum of the unsigned samples is 16 * 128 more
                int sg = 2048;
#pragma unroll
                for (int i = 0; i < 4; ++i) sg = __builtin_amdgcn_sdot4((int)pk[i], 0x01010101, sg, false);
                ssum = (uint32_t)sg;
                B = v4i{(int)pk[0], (int)pk[1], (int)pk[2], (int)pk[3]};
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) ssum = __builtin_amdgcn_sad_u8(pk[i], 0u, ssum);
                // level shift: sample - 128 as int8 == sample ^ 0x80
                B = v4i{(int)(pk[0] ^ 0x80808080u), (int)(pk[1] ^ 0x80808080u), (int)(pk[2] ^ 0x80808080u),
                        (int)(pk[3] ^ 0x80808080u)};
            }
            // the sum over the four row-pair lanes of a unit (lanes n, n + 16, n + 32, n + 48) without a trip through LDS:
            // v_permlane16_swap / v_permlane32_swap exchange rows of 16 / halves of 32 between two copies of the value
            {
                const auto r16 = __builtin_amdgcn_permlane16_swap(ssum, ssum, false, false);
                ssum = r16[0] + r16[1];
                const auto r32 = __builtin_amdgcn_permlane32_swap(ssum, ssum, false, false);
                ssum = r32[0] + r32[1];
            }

            // coefficient 0 is formed exactly after this loop, by the lane (n, gq == j) for unit 16j+n
            if (gq == (uint32_t)j) dcsum = ssum;

            bool amb = false;
            uint32_t nzlo = 0, nzhi = 0;  // this lane's part of the unit's non-zero mask
            uint32_t qprev[4];            // values of the even row tile, paired with the odd one for the mask
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                uint32_t qb[4];  // low 16 bits = quantised value
                // the scale factors and thresholds of this group were requested one group ago (they depend on the row tile only:
                // the four sets go round); read where they are used, the two LDS reads sit two instructions in front of their
                // first use and the wave waits out the LDS latency sixteen times per pass
                float qfr[8];
                {
                    const v4f qs = qf_s, qh = qf_h;
                    const float* nq = &s_qf[ct][4 * ((mt + 1) & 3) + gq][0];
                    qf_s = *reinterpret_cast<const v4f*>(nq);
                    qf_h = *reinterpret_cast<const v4f*>(nq + 4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) qfr[i] = qs[i], qfr[4 + i] = qh[i];
                }
                screen_quantise<STD>(A[mt], B, sp, qfr, ct, mt, gq, lane, qb, amb);
                // zig-zag positions 16mt+4gq .. +3 of unit 16j+n -> transpose buffer + non-zero bits
                i16a* row = tb16 + (16 * mt + 4 * gq) * 64 + row_unit_off(16 * j + n);
#pragma unroll
                for (int r = 0; r < 4; ++r) row[r * 64] = (int16_t)qb[r];
                // Non-zero bits, two values per instruction: the 16-bit values of row tiles mt - 1 and mt side by side
                // (one v_perm_b32), min(value, 1) on both halves (one v_pk_min_u16) = the flags at bits 0 and 16 --
                // exactly where positions 16 (mt - 1) + r and 16 mt + r sit in the mask word -- shifted in by r.
                if (mt & 1) {
                    uint32_t w = 0;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t pr = __builtin_amdgcn_perm(qb[r], qprev[r], 0x05040100u);  // qprev.lo16 | qb.lo16 << 16
                        uint32_t f;  // (the compiler turns min(x, 1) into two compares and two selects)
                        asm("v_pk_min_u16 %0, %1, 1 op_sel_hi:[1,0]" : "=v"(f) : "v"(pr));
                        w |= f << r;
                    }
                    if (mt == 1) nzlo = w;
                    else nzhi = w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) qprev[r] = qb[r];
                }
            }
            atomicOr(&s_mlo[16 * j + n], (nzlo << (4 * gq)) & ~1u);
            atomicOr(&s_mhi[16 * j + n], nzhi << (4 * gq));
            if (amb) atomicOr(&s_mlo[16 * j + n], 1u);  // bit 0 (coefficient 0 is never walked) = "undecided unit"
            STAMP(6);
        }
        if (p + pstep < pairs_total) {  // wave-uniform
            nxt = locate(p + pstep);
            request_first_rows(nxt);
        }
        {
            // exact coefficient 0 of unit 16*gq + n.  Strict: c0 = fl(sum * SCALE_00), q0 = round(c0 / Q0)
            // (utils.cpp:336,459).  Standard: row 0 of the true DCT is exactly 1/8,
            // q0 = round-half-away(sum / (8 Q0)) in integers.
            int q0;
            if constexpr (STD) {
                const int sl = (int)dcsum - 8192;
                const uint32_t Q0 = (uint32_t)(ct ? q0_chroma : q0_luma), a0 = (uint32_t)(sl < 0 ? -sl : sl);
                const int n0 = (int)((a0 + 4u * Q0) / (8u * Q0));
                q0 = sl < 0 ? -n0 : n0;
            } else {
                // (fp64, ~30 double-rate instructions per lane and pass -- and still faster than reading the 16321 possible
                // results from a table in memory: 251.8 against 256.9 Gpixel/s with the table, even with its request issued
                // in front of the next pass's rows, gpurun r4r / r4s)
                const double c0 = (double)((int)dcsum - 8192) * kScale00;
                q0 = (int)__builtin_round(c0 / (ct ? q0_chroma : q0_luma));
            }
            tb16[row_unit_off(16 * gq + n)] = (int16_t)q0;
        }
        __builtin_amdgcn_wave_barrier();
        STAMP(1);

        __builtin_amdgcn_s_setprio(0);
        // ---- walk phase: lane = block
        const uint32_t b = luma420 ? tile * 64 + 16 * chan + (lane >> 2) : tile * 64 + lane;  // block, or MCU in 4:2:0
        const bool active = b < g.N;
        if constexpr (!STD) {
            // Units with a coefficient the screen could not decide: the exact chain is the arbiter.
            const bool undecided = active && (s_mlo[lane] & 1u) != 0;
            uint64_t todo = __ballot(undecided);
            while (todo) {  // wave-uniform: one unit at a time, the whole wave on it
                const uint32_t ul = (uint32_t)__builtin_ctzll(todo);
                todo &= todo - 1;
                if (lane == 0) atomicAdd(&sp.stats[1], 1ull);
                const uint32_t ub = tile * 64 + ul, uby = ub / g.nbx, ubx = ub - uby * g.nbx;
                exact_unit_wave(f, g, chan, ubx, uby, sp.qd, reinterpret_cast<double*>(s_slot), tb16 + row_unit_off(ul), &s_mlo[ul],
                                &s_mhi[ul], lane);
            }
        }
        i16a* const row16 = tb16 + row_unit_off(lane);
        uint64_t mask = ((uint64_t)s_mhi[lane] << 32 | s_mlo[lane]) & ~1ull;
        const int dc = (int)row16[0];

        if constexpr (PROBE) {
            uint32_t* dst = sp.coefs + us_base / 64 * 2048 + lane;
#pragma unroll
            for (int pp = 0; pp < 32; ++pp)
                dst[pp * 64] = active ? (((uint32_t)(uint16_t)row16[2 * pp * 64]) | ((uint32_t)(uint16_t)row16[(2 * pp + 1) * 64] << 16)) : 0u;
        }

        Packer32<StoreLds> pkr(StoreLds{&s_slot[lane]});
        mask = mark_zero_runs(mask);  // ZRL positions become virtual non-zeros (after the probe dump above)
        const uint32_t maxcnt = wave_max((uint32_t)__popcll(mask));
        bool ok = walk_nonzeros<STD>(row16, mask, s_lut2[ct], s_act[ct], pkr, maxcnt, walk_general[ct]);
        n_general += walk_general[ct] ? 1u : 0u;
        const uint32_t aclen = pkr.bits();
        uint32_t nw = pkr.words();
        STAMP(2);
        const bool oversize = nw > kSlotRows;
        // (an error also poisons the tile's bit total -- bit 31, never reached by the sums -- which is how k_tile_scan
        // learns WHICH frame failed without this kernel carrying a per-frame flag array)
        if (!ok && active) atomicOr(sp.status, 1u), POISON_TILE();  // MI355_E_CATEGORY
        if (!active) nw = 0;

        // Total bits of the unit = DC symbol + AC string.  The DC difference needs the previous
        // block of the same channel: the neighbouring lane.  Lane 0's predecessor is the last block
        // of the previous tile, which another wave owns: its DC symbol is left out here and added
        // by k_dc_heads from the DCs in `meta`.  Tile sums are accumulated with one atomic per wave.
        uint32_t ubits = aclen;
        {
            const int pred = __builtin_amdgcn_update_dpp(0, dc, 0x138, 0xf, 0xf, false);  // wave_shr:1 -- the previous lane's DC, no trip through LDS
            auto count = [&](uint32_t, uint32_t len) { ubits += len; };
            const bool dc_ok = lane == 0 || put_dc(dc - pred, s_dc[ct], count);
            if (!dc_ok && active) atomicOr(sp.status, 1u), POISON_TILE();  // MI355_E_CATEGORY
            if (!active) ubits = 0;
        }
        STAMP(3);
        // arena space: regular strings back to back; oversized ones get a full-size private run.  ONE wave scan carries
        // both sums: the units' bits (< 2^11 each) in the low 20 bits, the words needed (<= 54 each) above them.
        const uint32_t need = oversize && nw ? kSlotWordsFull : nw;
        const uint32_t both = wave_incl_scan((need << 20) | ubits, lane);
        const uint32_t both_all = (uint32_t)__builtin_amdgcn_readlane((int)both, 63);
        if (lane == 0 && (both_all & 0xFFFFFu)) atomicAdd(&sp.tile_bits[(size_t)frame * g.tiles + tile], both_all & 0xFFFFFu);
        const uint32_t incl = both >> 20;
        const uint32_t base = wa.take(sp, both_all >> 20, lane);
        const uint32_t off = base + incl - need;
        const bool fits = base != 0xFFFFFFFFu;
        if (!fits) {
            // cannot happen: the overflow pool holds the worst case of every unit of the part (run_screened).  MI355_E_INTERNAL.
            if (lane == 0) atomicOr(sp.status, 4u), POISON_TILE();
        } else {
            const uint32_t ncopy = oversize ? 0u : nw;
            // the first eight words of every string are read from the slot unconditionally, back to back (the slot has 25
            // rows: always in bounds), and only the stores are predicated: read under its predicate, each word costs a full
            // LDS round trip in front of its store
            uint32_t sw[8];
#pragma unroll
            for (uint32_t w = 0; w < 8; ++w) sw[w] = s_slot[w * 64 + lane];
#pragma unroll
            for (uint32_t w = 0; w < 8; ++w)
                if (w < ncopy) sp.arena[off + w] = sw[w];
            for (uint32_t w = 8; wave_any(w < ncopy); w += 4) {  // (24 slot rows + the dump row: rows w .. w + 3 exist for w <= 20)
                uint32_t s4[4];
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) s4[i] = s_slot[(w + i) * 64 + lane];
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i)
                    if (w + i < ncopy) sp.arena[off + w + i] = s4[i];
            }
            const uint64_t again = __ballot(oversize && nw);
            if (again) {  // string longer than the LDS slot (q50: never; noise at q90: most luma units): walk again, straight to memory
                n_rewalked += (uint32_t)__popcll(again);
                if (oversize && nw) {
                    Packer32<StoreGlobal> pg(StoreGlobal{sp.arena + off});
                    bool gen = true;
                    (void)walk_nonzeros<STD>(row16, mask, s_lut2[ct], s_act[ct], pg, maxcnt, gen);
                }
            }
        }
        // 4 bytes per unit: the arena offset is not stored, k_merge forms it from the pass's base and a scan of the lengths
        sp.meta[us_base + lane] = active ? ((aclen << 16) | ((uint32_t)dc & 0xffffu)) : 0u;
        if (lane == 0) sp.pass_off[us_base >> 6] = base;
        __builtin_amdgcn_wave_barrier();
        STAMP(4);
        cur = nxt;
    }
    if (lane == 0 && n_rewalked) atomicAdd(&sp.stats[2], (unsigned long long)n_rewalked);
    if (lane == 0 && n_general) atomicAdd(&sp.stats[3], (unsigned long long)n_general);
#ifdef MI355_STAMPS
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(wave_t1)::"memory");
    if (sp.stamps && lane == 0) {
        for (int i = 0; i < 8; ++i) sp.stamps[(size_t)gwave * 8 + i] = stamp_sum[i];
        sp.stamps[(size_t)(2048 + gwave) * 8] = wave_t0;  // start / end of the wave, 10 ns ticks
        sp.stamps[(size_t)(2048 + gwave) * 8 + 1] = wave_t1;
    }
#endif
