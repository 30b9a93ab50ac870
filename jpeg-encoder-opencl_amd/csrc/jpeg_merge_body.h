// (Not a header: the body of two kernels, included inside their definitions -- see below.  Named .h so that the
// hash of the kernel sources, bench.kernel_sources_sha, covers it.)
// Body of the merge kernels k_merge<S420, SMALL> and k_gray_merge<SMALL>, included inside each kernel's definition
// (jpeg_screen_kernels.hip; why an include: jpeg_screen_encode_body.h).  In scope: the kernel parameters and the
// compile-time constants S420, SMALL, GRAY.
    constexpr uint32_t NT = S420 ? 384 : (GRAY ? 64 : 192), UPB = S420 ? 6 : (GRAY ? 1 : 3);  // threads, units per scan step (block / MCU)
    __builtin_amdgcn_s_setprio(3);  // see k_dc_heads
    // the 4:2:0 form gives up 256 window words for its longer offset array, so that both forms stay
    // within the 17.9 KiB a CU has left next to two resident workgroups of k_screen_encode
    constexpr uint32_t kWindow = (SMALL ? kEmitLdsWordsSmall : kEmitLdsWords) - (S420 ? 256 : 0);
    __shared__ uint32_t s_dc[2][16];
    __shared__ uint32_t s_bits[NT];
    __shared__ alignas(16) uint32_t s_words[kWindow];
    const uint32_t tid = threadIdx.x, lane = tid & 63, chan = GRAY ? 0u : tid >> 6;
    const uint32_t tile = blockIdx.x, frame = blockIdx.y;
    // a frame with an error (k_tile_scan wrote its verdict in place of the bit count: over capacity, a size without a
    // code) is skipped as a whole; the other frames of the call are written in full
    if (frame_bits[frame] >= kBitsFlagged) return;
    if (lds_words_limit > kWindow) lds_words_limit = kWindow;
    const uint32_t ft0 = frame * g.tiles;  // (slot indices in 32 bits: a part has fewer unit slots than arena words, and those are below 2^32)
    const uint64_t* to = tile_off + (size_t)frame * (g.tiles + 1);
    const uint64_t start = to[tile], end = to[tile + 1];
    const uint64_t w0 = start >> 5;
    const uint32_t nw = (uint32_t)(((end + 31) >> 5) - w0);
    const bool use_lds = nw <= lds_words_limit;
    uint32_t* outw = reinterpret_cast<uint32_t*>(out + (size_t)frame * out_stride);
    const bool last_tile = tile + 1 == g.tiles;
    const bool restart = (g.flags & 8u) != 0;          // MI355_F_RESTART
    const uint32_t ptile = restart ? 0u : tile;        // "no previous tile" for the DC predictors
    const uint32_t last_blk = g.N - 1 - tile * 64 < 63 ? g.N - 1 - tile * 64 : 63;  // last active block / MCU
    if (tid < 32) s_dc[tid >> 4][tid & 15] = lut[(tid >> 4) * 256 + (tid & 15)];
    if (use_lds) {  // (16 bytes per store; up to three words beyond nw: the window's size is a multiple of four)
        static_assert(kWindow % 4 == 0, "the window is zeroed and written out four words at a time");
        for (uint32_t i = tid * 4; i < nw; i += NT * 4) *reinterpret_cast<uint4*>(&s_words[i]) = make_uint4(0u, 0u, 0u, 0u);
    } else {
        for (uint32_t i = tid; i < nw; i += NT) {
            bool shared = (i == 0 && (start & 31)) || (i == nw - 1 && (end & 31) && !last_tile);
            if (!shared) __hip_atomic_store(&outw[w0 + i], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // this unit: DC, AC length, arena offset; the first words of its AC string are fetched now
    bool active, chroma, tile_end;  // tile_end: the last unit of the tile's scan
    uint32_t spos;  // position of the unit in the tile's scan
    uint32_t mw, moff;  // the unit's metadata word (aclen << 16 | dc) and the arena offset of its AC string
    int dc, pred;
    // Arena offsets are not stored per unit: a pass's strings lie back to back from the pass's base in lane order, so a
    // unit's offset is the base plus the words of the lanes in front of it -- one wave scan over the pass's 64 metadata words.
    auto words_of = [](uint32_t w) {
        const uint32_t nwz = ((w >> 16) + 31u) >> 5;
        return nwz > kSlotRows ? kSlotWordsFull : nwz;  // oversized strings own a full-size run (k_screen_encode)
    };
    if constexpr (S420) {
        const uint32_t mcu = tid / 6, k = tid - mcu * 6;
        const uint32_t t0 = (ft0 + tile) * 6 * 64;
        {   // wave w = pass w of the tile: offsets in pass order through s_bits, picked up in scan order below
            const uint32_t need = words_of(meta[t0 + tid]);
            s_bits[tid] = pass_off[(ft0 + tile) * 6 + (tid >> 6)] + wave_incl_scan_dpp(need) - need;
            __syncthreads();
        }
        spos = tid;
        chroma = k >= 4;
        active = tile * 64 + mcu < g.N;
        tile_end = mcu == last_blk && k == 5;
        pred = 0;
        if (!chroma) {
            const uint32_t L = 4 * mcu + k;  // pass L >> 6, lane L & 63: slot t0 + L
            mw = meta[t0 + L];
            moff = s_bits[L];
            if (L > 0) pred = meta_dc(meta[t0 + L - 1]);
            else if (ptile > 0) pred = meta_dc(meta[t0 - 6 * 64 + 3 * 64 + 63]);
        } else {
            const uint32_t slot = t0 + k * 64 + mcu;
            mw = meta[slot];
            moff = s_bits[k * 64 + mcu];
            if (mcu > 0) pred = meta_dc(meta[slot - 1]);
            else if (ptile > 0) pred = meta_dc(meta[slot - 6 * 64 + 63]);
        }
        dc = meta_dc(mw);
    } else {
        spos = lane * UPB + chan;
        chroma = chan != 0;
        active = tile * 64 + lane < g.N;
        tile_end = lane == last_blk && chan == UPB - 1;
        mw = meta[((ft0 + tile) * UPB + chan) * 64 + lane];
        const uint32_t need = words_of(mw);
        moff = pass_off[(ft0 + tile) * UPB + chan] + wave_incl_scan_dpp(need) - need;
        dc = meta_dc(mw);
        pred = meta_pred<UPB>(meta, ft0, ptile, chan, lane, dc);
        if (restart && lane == 0) pred = 0;
    }
    const uint32_t aclen = active ? (mw >> 16) : 0u;
    // the first four words of the string in ONE load (dword-aligned; the words behind a shorter string are read and not used:
    // the arena ends in more than a kilobyte of slack per wave region)
    struct __attribute__((packed, aligned(4))) Words4 {
        uint32_t w[4];
    };
    uint32_t pre[4] = {0u, 0u, 0u, 0u};
    if (aclen) {
        const Words4 p4 = *reinterpret_cast<const Words4*>(arena + moff);
#pragma unroll
        for (int i = 0; i < 4; ++i) pre[i] = p4.w[i];
    }
    __syncthreads();
    // tile-local exclusive offsets in scan order; the DC symbol is formed once and kept (code | value bits, right-aligned)
    uint32_t dsym = 0, dcl = 0;
    {
        auto keep = [&](uint32_t code, uint32_t len) { dsym = code, dcl = len; };
        put_dc(dc - pred, s_dc[chroma ? 1 : 0], keep);
    }
    s_bits[spos] = active ? dcl + aclen : 0u;
    __syncthreads();
    if (tid < 64) {
        uint32_t a[UPB], sum = 0;
#pragma unroll
        for (uint32_t i = 0; i < UPB; ++i) a[i] = s_bits[tid * UPB + i], sum += a[i];
        uint32_t run = wave_incl_scan_dpp(sum) - sum;
#pragma unroll
        for (uint32_t i = 0; i < UPB; ++i) {
            s_bits[tid * UPB + i] = run;
            run += a[i];
        }
    }
    __syncthreads();
    if (active) {
        // The unit's bits go into the (zeroed) window by OR, a word at a time: the DC symbol at its bit position, then the
        // AC string -- whole words as they lie in the arena (left-aligned, zero beyond the string's end), each funnelled
        // with its predecessor to the string's bit phase: one v_alignbit_b32 and one LDS OR per word, no 64-bit
        // accumulator, no length bookkeeping.  (This kernel's instructions are issued on the SIMDs the block encode of the
        // next part runs on: until round 4 it took 270 vector and 200 scalar instructions per wave of 64 units, an eighth of
        // the encode kernel's own.)
        const uint32_t pos = (uint32_t)(start & 31) + s_bits[spos];  // bits from the first word of the tile: below 2^21
        // restart intervals end on a byte boundary, filled with 1s (their start is aligned)
        const uint32_t fill = restart && tile_end ? (8u - ((pos + dcl + aclen) & 7u)) & 7u : 0u;
        auto body = [&](auto&& orw) {
            if (dcl) {
                const uint32_t d = dsym << (32u - dcl), sh = pos & 31u;  // left-aligned; dcl <= 27
                orw(pos >> 5, d >> sh);
                if (sh + dcl > 32u) orw((pos >> 5) + 1u, d << (32u - sh));
            }
            const uint32_t pa = pos + dcl, sa = pa & 31u, ja = pa >> 5;
            uint32_t prev = 0;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                if (i * 32u < aclen) {
                    orw(ja + i, __builtin_amdgcn_alignbit(prev, pre[i], sa));  // (prev : word) >> sa
                    prev = pre[i];
                }
            }
            for (uint32_t k = 4; k * 32u < aclen; ++k) {
                const uint32_t w = arena[moff + k];
                orw(ja + k, __builtin_amdgcn_alignbit(prev, w, sa));
                prev = w;
            }
            // what the shift pushed out of the string's last word (its ((aclen - 1) & 31) + 1 valid bits reach beyond bit 31)
            if (aclen && ((aclen - 1u) & 31u) + sa >= 32u) orw(ja + ((aclen + 31u) >> 5), prev << (32u - sa));
            if (fill) {
                const uint32_t e = pa + aclen;
                orw(e >> 5, (((1u << fill) - 1u) << (32u - fill)) >> (e & 31u));
            }
        };
        if (use_lds) body([&](uint32_t j, uint32_t v) { atomicOr(&s_words[j], v); });
        else body([&](uint32_t j, uint32_t v) { atomicOr(&outw[w0 + j], __builtin_bswap32(v)); });
    }
    if (!use_lds) return;
    __syncthreads();
    // write-out, four words per thread and trip: one 16-byte LDS read, one 16-byte store where all four words are the
    // tile's own (every group but the first and the last); the words a tile shares with its neighbours go by atomic OR
    struct __attribute__((packed, aligned(4))) Out4 {
        uint32_t w[4];
    };
    const bool share_first = (start & 31) != 0, share_last = (end & 31) != 0 && !last_tile;
    for (uint32_t i = tid * 4; i < nw; i += NT * 4) {
        const uint4 r = *reinterpret_cast<const uint4*>(&s_words[i]);
        const uint32_t v[4] = {__builtin_bswap32(r.x), __builtin_bswap32(r.y), __builtin_bswap32(r.z), __builtin_bswap32(r.w)};
        if (i > 0 && i + 4 < nw) {
            *reinterpret_cast<Out4*>(&outw[w0 + i]) = Out4{{v[0], v[1], v[2], v[3]}};
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                const uint32_t w = i + k;
                if (w >= nw) break;
                const bool shared = (w == 0 && share_first) || (w == nw - 1 && share_last);
                if (shared) {
                    if (v[k]) atomicOr(&outw[w0 + w], v[k]);
                } else {
                    outw[w0 + w] = v[k];
                }
            }
        }
    }
