// Field-space loss of the spatial decoder (gfx950): sea_decode_mse.  The second decoder layer, the masked mean-squared error against the
// patch targets and the data gradient back to the hidden rows in ONE launch (plus a one-block finish that sums the loss partials):
//     Y = H W2^T + bias;   D = valid ? Y - target : 0;   loss = inv_n sum D^2;   dH = 2 grad_scale inv_n (D W2) [* GELU'(Z)]
// Y and D are never stored: W2 is the operand of BOTH products (contracted over the hidden index s in the first, over the output column c in
// the second), so a [rows, columns] tile lives only in the accumulator registers between two MFMA stages — the shape of a flash-attention
// backward with W2 as K and V at once.
//
// Tiling.  A workgroup (4 waves) owns 64 rows of one field group, wave w the rows 16 w .. 16 w + 15.  Each wave keeps its rows of H as MFMA
// fragments in registers (SP / 8 per lane) and its [16, SP] slice of dH as fp32 accumulators (SP / 4 per lane: 160 at SP = 640, which with the
// 80 fragment registers and the staging set fits the 512-register file at one wave per SIMD).  The workgroup walks the 32-row tiles of W2
// (32 output columns of one field; tiles that lie wholly in the pad columns [C, Cp) are skipped).  A tile is fetched once per workgroup — from
// L2, every workgroup of the launch reads the same few hundred kB — into one of two LDS images [32][SP] with a pitch of 2 SP + 32 bytes, through
// registers: the loads of tile t + 1 are issued before the MFMAs of tile t and stored after them, one barrier per tile.  Per tile and wave:
//   stage 1  Y^T[c, m] = sum_s W2[c, s] H[m, s]: W2 rows are the A operand (ds_read_b128, row c = lane & 15), the H fragments the B operand.  Two
//            16-column sub-tiles, two accumulators each (even / odd k-steps), start from the bias.  The result has the row m on the lane and four
//            consecutive columns c = 4 g + r in its registers,
//   between  which is how the target is read (one float4 per lane and sub-tile, each element exactly once, requested before stage 1), the residual
//            masked (select, so that a NaN or a huge value in an invalid slot is neutral), squared into the lane's loss sum, and rounded to bf16 ONCE,
//            as the composed path rounds dY when its GEMM reads it.  The 8 values are the A fragment of stage 2 with k-slot (g, j) = column
//            4 g + j (j < 4) or 16 + 4 g + j - 4,
//   stage 2  dH[m, s] += sum_c D[m, c] W2[c, s]: the SAME LDS image read column-wise — two ds_read_b64_tr_b16 per 16 hidden columns deliver rows
//            4 g .. 4 g + 3 and 16 + 4 g .. 16 + 4 g + 3 of the tile for column s = 16 st + (lane & 15): the k-slots above.
// The pitch of 8 dwords mod 64 banks keeps both read forms conflict-free (the 16 rows of a b128 read land on 16 distinct 16-byte bank groups, the 8
// rows of a 32-lane half of a transposed read on 8 distinct 32-byte ones).
//
// The hidden width is padded to SP in {128, 256, 384, 512, 640} by MASKING in the kernel, not in the shadow copies: H fragments and LDS chunks at
// s >= S are zero (S % 8 == 0: a 16-byte chunk is wholly inside or outside), k-steps and column tiles at or beyond S are skipped (uniform branches:
// the transposed reads need every lane active), dH stores are guarded by s < S.  Rows >= M hold zero fragments and a zero column limit; they take
// part in every barrier and cross-lane read and store nothing.
//
// Loss: lane sums -> wave -> workgroup in a fixed order, one partial per workgroup, summed by the finish block in a fixed order; dH has one
// writer per element.  No atomics: two runs give the same bits.
//
// What bounds it: per tile a wave issues 4 SP / 32 MFMAs (16x16x32) and reads the tile twice from LDS; with four waves per CU the LDS array
// (256 B / clk) is busy about as long as the matrix cores, so the launch sits near half the bf16 MFMA rate at best, and the 64-row block leaves one
// wave per SIMD (DESIGN.md section 7 has the measurements).
#include "sea_common.hpp"
#include "verify_score.hpp"   // sea_decode_member_verify scores a cell as verify_kernel scores a sensor
#include "quantile_select.hpp"   // sea_decode_member_quantiles reads a column out
#include "brier_score.hpp"       // sea_decode_member_brier scores a cell as brier_kernel scores a sensor

typedef short dm_s16x4 __attribute__((ext_vector_type(4)));

struct DecodeMseLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeMse p;
};

constexpr int DM_ROWS = 64;   // rows per workgroup
constexpr int DM_TC = 32;     // W2 rows (output columns) per tile
constexpr int DM_PAD = 32;    // bytes added to an LDS row

template <int SP>
constexpr int dm_lds_bytes() { return 2 * DM_TC * (SP * 2 + DM_PAD) + 16; }

// Tile t of a group (32 rows of W2: output columns [cb, cb + 32) of field j) into the thread's SP / 64 staging registers, chunks at s >= S zeroed; and on into an LDS image.
// (NT: threads of the workgroup; a thread carries DM_TC * (SP / 8) / NT chunks.)
template <int SP, int NT = 256>
__device__ __forceinline__ void dm_load_tile(uint4 (&wr)[SP * 4 / NT], const __bf16* W2, int ldw, int S, int Cp, int tpf, int t, int tid) {
    constexpr int CPR = SP / 8;
    const int j = t / tpf, cb = (t - j * tpf) * DM_TC;
    const __bf16* src = W2 + (int64_t)(j * Cp + cb) * ldw;
#pragma unroll
    for (int u = 0; u < SP * 4 / NT; ++u) {
        const int q = u * NT + tid, r = q / CPR, ch = q - r * CPR;
        wr[u] = ch * 8 < S ? *reinterpret_cast<const uint4*>(src + (int64_t)r * ldw + ch * 8) : make_uint4(0u, 0u, 0u, 0u);
    }
}
template <int SP, int NT = 256>
__device__ __forceinline__ void dm_store_tile(const uint4 (&wr)[SP * 4 / NT], char* buf, int tid) {
    constexpr int CPR = SP / 8, PITCH = SP * 2 + DM_PAD;
#pragma unroll
    for (int u = 0; u < SP * 4 / NT; ++u) {
        const int q = u * NT + tid, r = q / CPR, ch = q - r * CPR;
        *reinterpret_cast<uint4*>(buf + r * PITCH + ch * 16) = wr[u];
    }
}

template <int SP>
__global__ __launch_bounds__(256) void decode_mse_kernel(const DecodeMseLaunch L) {
    constexpr int KS = SP / 32;               // k-steps of stage 1
    constexpr int ST = SP / 16;               // hidden-column tiles of stage 2
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int CPR = SP / 8;               // 16-byte chunks per tile row
    constexpr int NCH = DM_TC * CPR / 256;    // chunks per thread
    static_assert(NCH * 256 == DM_TC * CPR, "whole chunks per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images, then 4 floats of the loss reduction
    float* red = reinterpret_cast<float*>(smem + 2 * TILE);

    const SeaDecodeMseGroup& G = L.g[blockIdx.y];
    const SeaDecodeMse& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int M = P.M, S = P.S, C = P.C, Cp = P.Cp;
    const int row0 = blockIdx.x * DM_ROWS + wave * 16;
    const int m = row0 + li;   // the row this lane holds in the H fragments, in the stage-1 result and in the residual fragment
    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);

    // valid columns of this lane's row: [0, lim)
    int lim = 0;
    if (m < M) {
        lim = C;
        if (P.counts != nullptr) {
            const int cnt = P.counts[m % P.P];
            lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
        }
    }

    uint4 hf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int s = ks * 32 + 8 * lg;
        hf[ks] = (m < M && s < S) ? *reinterpret_cast<const uint4*>(H + (int64_t)m * G.ldh + s) : zero4;
    }
    f32x4 dh[ST];
#pragma unroll
    for (int st = 0; st < ST; ++st) dh[st] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int tpf = (C + DM_TC - 1) / DM_TC;   // tiles of a field that hold real columns
    const int n_tiles = G.n_fields * tpf;
    uint4 wr[NCH];
    dm_load_tile<SP>(wr, W2, G.ldw, S, Cp, tpf, 0, tid);
    dm_store_tile<SP>(wr, smem, tid);
    __syncthreads();

    float lsum = 0.f;
    const float* trow = P.target + (int64_t)(m < M ? m : 0) * P.ld_row;
    typedef dm_s16x4 __attribute__((address_space(3))) * lds_p;
    for (int t = 0; t < n_tiles; ++t) {
        const char* buf = smem + (t & 1) * TILE;
        if (t + 1 < n_tiles) dm_load_tile<SP>(wr, W2, G.ldw, S, Cp, tpf, t + 1, tid);
        const int j = t / tpf, cb = (t - j * tpf) * DM_TC;

        // target of this lane's 2 x 4 columns (requested now, used after stage 1)
        float tg[2][4];
        const float* tf = trow + (int64_t)(G.field0 + j) * P.ld_field;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int c = cb + sub * 16 + 4 * lg;
            tg[sub][0] = tg[sub][1] = tg[sub][2] = tg[sub][3] = 0.f;
            if (c < lim) {
                if (c + 4 <= C) {
                    const float4 v = *reinterpret_cast<const float4*>(tf + c);
                    tg[sub][0] = v.x; tg[sub][1] = v.y; tg[sub][2] = v.z; tg[sub][3] = v.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (c + r < C) tg[sub][r] = tf[c + r];
                }
            }
        }

        // stage 1
        f32x4 acc[2][2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const float4 b = *reinterpret_cast<const float4*>(G.bias + j * Cp + cb + sub * 16 + 4 * lg);
            acc[sub][0] = f32x4{b.x, b.y, b.z, b.w};
            acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks * 32 < S) {
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    const uint4 a = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                    mma16<__bf16>(a, hf[ks], acc[sub][ks & 1]);
                }
            }
        }

        // residual: masked, squared into the loss, rounded once
        bf16x8 dfr;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = cb + sub * 16 + 4 * lg + r;
                const float y = acc[sub][0][r] + acc[sub][1][r];
                const float d = c < lim ? y - tg[sub][r] : 0.f;
                lsum = fma1(d, d, lsum);
                dfr[sub * 4 + r] = (__bf16)d;
            }
        }
        const uint4 da = __builtin_bit_cast(uint4, dfr);

        // stage 2
        const char* tb = buf + (4 * lg + (li >> 2)) * PITCH + (4 * (li & 3)) * 2;
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            if (st * 16 < S) {
                const dm_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(tb + st * 32));
                const dm_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(tb + st * 32 + 16 * PITCH));
                const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                mma16<__bf16>(da, make_uint4(l2.x, l2.y, h2.x, h2.y), dh[st]);
            }
        }

        if (t + 1 < n_tiles) dm_store_tile<SP>(wr, smem + ((t + 1) & 1) * TILE, tid);
        __syncthreads();
    }

    // dH: register r of tile st is row 4 g + r of the wave, column 16 st + (lane & 15)
    const float scale = 2.0f * P.grad_scale * P.inv_n;
    __bf16* dH = static_cast<__bf16*>(G.dH);
    const __bf16* Z = static_cast<const __bf16*>(G.Z);
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        const int s = st * 16 + li;
        if (s < S) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mr = row0 + 4 * lg + r;
                if (mr < M) {
                    float v = dh[st][r] * scale;
                    if (Z != nullptr) v *= gelu_grad_for<__bf16>((float)Z[(int64_t)mr * G.ldz + s]);
                    dH[(int64_t)mr * G.lddh + s] = (__bf16)v;
                }
            }
        }
    }

    lsum = wave_sum(lsum);
    if (lane == 0) red[wave] = lsum;
    __syncthreads();
    if (tid == 0) P.partial[blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// loss = inv_n * sum(partial), summed in a fixed order (one block)
__global__ __launch_bounds__(256) void decode_mse_finish_kernel(const float* __restrict__ partial, int n_partial, float* __restrict__ loss, float inv_n) {
    __shared__ float red[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) * inv_n;
}

template <int SP>
static int decode_mse_launch(const DecodeMseLaunch& L, dim3 grid, hipStream_t s) {
    constexpr int lds = dm_lds_bytes<SP>();
    static const hipError_t once = hipFuncSetAttribute(reinterpret_cast<const void*>(decode_mse_kernel<SP>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)once;
    decode_mse_kernel<SP><<<grid, dim3(256), lds, s>>>(L);
    return 0;
}

extern "C" int sea_decode_mse(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMse* p, int dtype, void* stream) {
    SEA_REQUIRE(groups != nullptr && p != nullptr, "sea_decode_mse: null argument table");
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "sea_decode_mse: n_groups=%d outside 1..%d", n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "sea_decode_mse: bad dtype %d", dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("sea_decode_mse: unsupported: bf16 only (the fp32 decoder composes sea_gemm_grouped and sea_mse_fwd_bwd)");
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeMse& P = *p;
    SEA_REQUIRE(P.target != nullptr && P.loss != nullptr && P.partial != nullptr, "sea_decode_mse: null target, loss or partial pointer");
    SEA_REQUIRE(P.M >= 1, "sea_decode_mse: M=%d must be positive", P.M);
    SEA_REQUIRE(P.S >= 8 && P.S % 8 == 0, "sea_decode_mse: S=%d must be a positive multiple of 8", P.S);
    SEA_REQUIRE(P.Cp >= 32 && P.Cp % 32 == 0, "sea_decode_mse: Cp=%d must be a positive multiple of 32", P.Cp);
    SEA_REQUIRE(P.C >= 1 && P.C <= P.Cp, "sea_decode_mse: C=%d must lie in 1..Cp=%d", P.C, P.Cp);
    SEA_REQUIRE(P.P >= 1, "sea_decode_mse: P=%d must be positive", P.P);
    SEA_REQUIRE(P.counts == nullptr || P.M % P.P == 0, "sea_decode_mse: M=%d is not a multiple of P=%d (counts given)", P.M, P.P);
    SEA_REQUIRE(P.ld_row >= 0 && P.ld_row % 4 == 0 && P.ld_field >= 0 && P.ld_field % 4 == 0,
                "sea_decode_mse: target strides ld_row=%lld, ld_field=%lld must be multiples of 4", (long long)P.ld_row, (long long)P.ld_field);
    SEA_REQUIRE(sea_aligned16(P.target) && sea_aligned4(P.counts) && sea_aligned4(P.loss) && sea_aligned4(P.partial), "sea_decode_mse: misaligned target, counts, loss or partial pointer");
    for (int g = 0; g < n_groups; ++g) {
        const SeaDecodeMseGroup& G = groups[g];
        SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr && G.dH != nullptr, "sea_decode_mse: group %d: null pointer", g);
        SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias) && sea_aligned16(G.dH) && sea_aligned16(G.Z), "sea_decode_mse: group %d: pointers must be 16-byte aligned", g);
        SEA_REQUIRE(G.ldh >= P.S && G.ldh % 8 == 0 && G.ldw >= P.S && G.ldw % 8 == 0 && G.lddh >= P.S && G.lddh % 2 == 0 && (G.Z == nullptr || G.ldz >= P.S),
                    "sea_decode_mse: group %d: row strides ldh=%d ldw=%d lddh=%d ldz=%d must cover S=%d (ldh, ldw multiples of 8)", g, G.ldh, G.ldw, G.lddh, G.ldz, P.S);
        SEA_REQUIRE(G.n_fields >= 1 && G.field0 >= 0, "sea_decode_mse: group %d: n_fields=%d, field0=%d", g, G.n_fields, G.field0);
        SEA_REQUIRE((int64_t)G.n_fields * P.Cp <= 0x7fffffffLL / 2, "sea_decode_mse: group %d: too many output columns", g);
    }
    if (P.S > 640) {
        sea_set_error("sea_decode_mse: unsupported: hidden width S=%d above 640", P.S);
        return SEA_EUNSUPPORTED;
    }
    const int64_t row_blocks = ((int64_t)P.M + DM_ROWS - 1) / DM_ROWS;
    SEA_REQUIRE(row_blocks * n_groups <= 0x7fffffffLL && row_blocks <= 0x7fffffffLL, "sea_decode_mse: too many rows");
    SEA_REQUIRE((int64_t)P.n_partial_cap >= row_blocks * n_groups, "sea_decode_mse: partial workspace of %d floats is too small: %lld needed (ceil(M / 64) * n_groups)",
                P.n_partial_cap, (long long)(row_blocks * n_groups));

    DecodeMseLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)row_blocks, (unsigned)n_groups);
    if (P.S <= 128) decode_mse_launch<128>(L, grid, s);
    else if (P.S <= 256) decode_mse_launch<256>(L, grid, s);
    else if (P.S <= 384) decode_mse_launch<384>(L, grid, s);
    else if (P.S <= 512) decode_mse_launch<512>(L, grid, s);
    else decode_mse_launch<640>(L, grid, s);
    decode_mse_finish_kernel<<<dim3(1), dim3(256), 0, s>>>(P.partial, (int)(row_blocks * n_groups), P.loss, P.inv_n);
    SEA_CHECK_LAUNCH("sea_decode_mse");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_member_sse: the per-member, per-field squared error of the decoded fields against an observation (ensemble weighting).  Stage 1 of
// decode_mse_kernel — the same W2 tiles through the same two LDS images, the same H fragments in registers — with another epilogue and no stage 2:
// the residual is squared in fp32 where it is produced and summed per ROW and FIELD.  A lane holds one row (m = row0 + lane & 15) and 8 of a tile's 32
// columns; it adds its squares over the tiles of a field in a fixed order, the four lanes that share the row (lane >> 4) are folded by two butterfly
// steps, and the lane group 0 writes work[m, field0 + j]: one writer per element.  A row tile may straddle members (P is arbitrary), so the P rows of a
// member are summed by member_sse_finish_kernel — one wave per output element, lanes over the patches, a fixed butterfly — and not in the main kernel.
// Without the dH accumulators a wave needs SP / 8 fragment registers and little else, so a workgroup is NW waves = 16 NW rows with NW in {4, 8}: at
// NW = 8 every W2 tile is fetched from L2 and written to LDS half as often per row and two waves share a SIMD (at SP = 640 the two LDS images are
// 84 kB: one workgroup per CU either way).  The entry point picks NW (measured: 128 rows above S = 512, 64 below; SEA_TUNE sse_rows=64|128 forces one; both give the same bits).
struct MemberSseLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeMemberSse p;
};

template <int SP, int NW>
__global__ __launch_bounds__(64 * NW) void decode_member_sse_kernel(const MemberSseLaunch L) {
    constexpr int NT = 64 * NW;
    constexpr int KS = SP / 32;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images

    const SeaDecodeMseGroup& G = L.g[blockIdx.y];
    const SeaDecodeMemberSse& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int M = P.M, S = P.S, C = P.C, Cp = P.Cp;
    const int row0 = blockIdx.x * (16 * NW) + wave * 16;
    const int m = row0 + li;
    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);

    // valid columns of this lane's row: [0, lim); its row of the observation: the `members` consecutive members of a history share one
    int lim = 0;
    int64_t tr = 0;
    if (m < M) {
        const int mem = m / P.P, patch = m - mem * P.P;
        lim = C;
        if (P.counts != nullptr) {
            const int cnt = P.counts[patch];
            lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
        }
        tr = (int64_t)(mem / P.members) * P.P + patch;
    }

    uint4 hf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int s = ks * 32 + 8 * lg;
        hf[ks] = (m < M && s < S) ? *reinterpret_cast<const uint4*>(H + (int64_t)m * G.ldh + s) : zero4;
    }

    const int tpf = (C + DM_TC - 1) / DM_TC;
    const int n_tiles = G.n_fields * tpf;
    uint4 wr[NCH];
    dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, 0, tid);
    dm_store_tile<SP, NT>(wr, smem, tid);
    __syncthreads();

    float fsum = 0.f;
    const float* trow = P.target + tr * P.ld_row;
    float* wrow = P.work + (int64_t)(m < M ? m : 0) * P.n_fields_total + G.field0;
    int j = 0, tj = 0;   // field of tile t and the tile's index inside it
    for (int t = 0; t < n_tiles; ++t) {
        const char* buf = smem + (t & 1) * TILE;
        if (t + 1 < n_tiles) dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t + 1, tid);
        const int cb = tj * DM_TC;

        float tg[2][4];
        const float* tf = trow + (int64_t)(G.field0 + j) * P.ld_field;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int c = cb + sub * 16 + 4 * lg;
            tg[sub][0] = tg[sub][1] = tg[sub][2] = tg[sub][3] = 0.f;
            if (c < lim) {
                if (c + 4 <= C) {
                    const float4 v = *reinterpret_cast<const float4*>(tf + c);
                    tg[sub][0] = v.x; tg[sub][1] = v.y; tg[sub][2] = v.z; tg[sub][3] = v.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (c + r < C) tg[sub][r] = tf[c + r];
                }
            }
        }

        f32x4 acc[2][2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const float4 b = *reinterpret_cast<const float4*>(G.bias + j * Cp + cb + sub * 16 + 4 * lg);
            acc[sub][0] = f32x4{b.x, b.y, b.z, b.w};
            acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks * 32 < S) {
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    const uint4 a = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                    mma16<__bf16>(a, hf[ks], acc[sub][ks & 1]);
                }
            }
        }

        // residual: masked (a select: NaN in an invalid slot is neutral), squared in fp32, never rounded
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = cb + sub * 16 + 4 * lg + r;
                const float y = acc[sub][0][r] + acc[sub][1][r];
                const float d = c < lim ? y - tg[sub][r] : 0.f;
                fsum = fma1(d, d, fsum);
            }
        }
        if (++tj == tpf) {   // the field is complete (uniform over the workgroup): fold the row's four lanes, one writer
            float v = fsum;
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lg == 0 && m < M) wrow[j] = v;
            fsum = 0.f;
            tj = 0;
            ++j;
        }

        if (t + 1 < n_tiles) dm_store_tile<SP, NT>(wr, smem + ((t + 1) & 1) * TILE, tid);
        __syncthreads();
    }
}

// sse[member, f] = sum over the member's P rows of work[row, f]: one wave per output element, lane l adds the rows l, l + 64, .. in order, then a fixed butterfly
__global__ __launch_bounds__(256) void member_sse_finish_kernel(const float* __restrict__ work, float* __restrict__ sse, int64_t n_out, int P, int nft) {
    const int lane = threadIdx.x & 63;
    const int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= n_out) return;   // whole waves leave: no barrier follows
    const int64_t mem = o / nft;
    const int f = (int)(o - mem * nft);
    const float* src = work + mem * P * nft + f;
    float acc = 0.f;
    for (int p = lane; p < P; p += 64) acc += src[(int64_t)p * nft];
    acc = wave_sum(acc);
    if (lane == 0) sse[o] = acc;
}

template <int SP, int NW>
static void member_sse_launch(const MemberSseLaunch& L, int64_t M, int n_groups, hipStream_t s) {
    constexpr int lds = 2 * DM_TC * (SP * 2 + DM_PAD);
    static bool set_on[64] = {false};   // per device: SP = 640 needs 84 kB, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_member_sse_kernel<SP, NW>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    const dim3 grid((unsigned)((M + 16 * NW - 1) / (16 * NW)), (unsigned)n_groups);
    decode_member_sse_kernel<SP, NW><<<grid, dim3(64 * NW), lds, s>>>(L);
}

template <int NW>
static void member_sse_dispatch(const MemberSseLaunch& L, int n_groups, hipStream_t s) {
    const int S = L.p.S;
    const int64_t M = L.p.M;
    if (S <= 128) member_sse_launch<128, NW>(L, M, n_groups, s);
    else if (S <= 256) member_sse_launch<256, NW>(L, M, n_groups, s);
    else if (S <= 384) member_sse_launch<384, NW>(L, M, n_groups, s);
    else if (S <= 512) member_sse_launch<512, NW>(L, M, n_groups, s);
    else member_sse_launch<640, NW>(L, M, n_groups, s);
}

extern "C" int sea_decode_member_sse(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberSse* p, int dtype, void* stream) {
    SEA_REQUIRE(groups != nullptr && p != nullptr, "sea_decode_member_sse: null argument table");
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "sea_decode_member_sse: n_groups=%d outside 1..%d", n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "sea_decode_member_sse: bad dtype %d", dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("sea_decode_member_sse: unsupported: bf16 only (the fp32 decoder composes sea_gemm_grouped and reductions)");
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeMemberSse& P = *p;
    SEA_REQUIRE(P.target != nullptr && P.sse != nullptr && P.work != nullptr, "sea_decode_member_sse: null target, sse or work pointer");
    SEA_REQUIRE(P.M >= 1, "sea_decode_member_sse: M=%d must be positive", P.M);
    SEA_REQUIRE(P.S >= 8 && P.S % 8 == 0, "sea_decode_member_sse: S=%d must be a positive multiple of 8", P.S);
    SEA_REQUIRE(P.Cp >= 32 && P.Cp % 32 == 0, "sea_decode_member_sse: Cp=%d must be a positive multiple of 32", P.Cp);
    SEA_REQUIRE(P.C >= 1 && P.C <= P.Cp, "sea_decode_member_sse: C=%d must lie in 1..Cp=%d", P.C, P.Cp);
    SEA_REQUIRE(P.P >= 1 && P.members >= 1, "sea_decode_member_sse: P=%d and members=%d must be positive", P.P, P.members);
    SEA_REQUIRE((int64_t)P.M % ((int64_t)P.P * P.members) == 0, "sea_decode_member_sse: M=%d is not a multiple of P * members = %d * %d", P.M, P.P, P.members);
    SEA_REQUIRE(P.n_fields_total >= 1, "sea_decode_member_sse: n_fields_total=%d must be positive", P.n_fields_total);
    SEA_REQUIRE(P.work_cap >= (int64_t)P.M * P.n_fields_total, "sea_decode_member_sse: workspace of %lld floats is too small: %lld needed (M * n_fields_total)",
                (long long)P.work_cap, (long long)((int64_t)P.M * P.n_fields_total));
    SEA_REQUIRE(P.ld_row >= 0 && P.ld_row % 4 == 0 && P.ld_field >= 0 && P.ld_field % 4 == 0,
                "sea_decode_member_sse: target strides ld_row=%lld, ld_field=%lld must be multiples of 4", (long long)P.ld_row, (long long)P.ld_field);
    SEA_REQUIRE(sea_aligned16(P.target) && sea_aligned4(P.counts) && sea_aligned4(P.sse) && sea_aligned4(P.work), "sea_decode_member_sse: misaligned target, counts, sse or work pointer");
    int64_t covered = 0;
    for (int g = 0; g < n_groups; ++g) {
        const SeaDecodeMseGroup& G = groups[g];
        SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr, "sea_decode_member_sse: group %d: null pointer", g);
        SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias), "sea_decode_member_sse: group %d: pointers must be 16-byte aligned", g);
        SEA_REQUIRE(G.ldh >= P.S && G.ldh % 8 == 0 && G.ldw >= P.S && G.ldw % 8 == 0,
                    "sea_decode_member_sse: group %d: row strides ldh=%d ldw=%d must cover S=%d and be multiples of 8", g, G.ldh, G.ldw, P.S);
        SEA_REQUIRE(G.n_fields >= 1 && G.field0 >= 0 && (int64_t)G.field0 + G.n_fields <= P.n_fields_total,
                    "sea_decode_member_sse: group %d: n_fields=%d, field0=%d outside the %d fields", g, G.n_fields, G.field0, P.n_fields_total);
        SEA_REQUIRE((int64_t)G.n_fields * P.Cp <= 0x7fffffffLL / 2, "sea_decode_member_sse: group %d: too many output columns", g);
        for (int h = 0; h < g; ++h)
            SEA_REQUIRE(G.field0 >= groups[h].field0 + groups[h].n_fields || groups[h].field0 >= G.field0 + G.n_fields,
                        "sea_decode_member_sse: group %d: its fields overlap those of group %d (every output element has one writer)", g, h);
        covered += G.n_fields;
    }
    SEA_REQUIRE(covered == P.n_fields_total, "sea_decode_member_sse: the groups cover %lld of the %d fields (every field needs exactly one group)", (long long)covered, P.n_fields_total);
    if (P.S > 640) {
        sea_set_error("sea_decode_member_sse: unsupported: hidden width S=%d above 640", P.S);
        return SEA_EUNSUPPORTED;
    }
    const int64_t n_out = (int64_t)(P.M / P.P) * P.n_fields_total;
    SEA_REQUIRE(((int64_t)P.M + 63) / 64 <= 0x7fffffffLL && (n_out + 3) / 4 <= 0x7fffffffLL, "sea_decode_member_sse: too many rows");

    MemberSseLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    hipStream_t s = static_cast<hipStream_t>(stream);
    // measured (tools/ensemble_bench.py): at SP = 640 the two LDS images leave one workgroup per CU and 128 rows are 1.4x faster;
    // up to SP = 512 two workgroups fit and 64 rows are 3 - 9 % faster.  Read per call: the tool measures both forms in one process.
    const int rows = sea_tune("sse_rows", P.S > 512 ? 128 : 64);
    if (rows == 64) member_sse_dispatch<4>(L, n_groups, s);
    else member_sse_dispatch<8>(L, n_groups, s);
    member_sse_finish_kernel<<<dim3((unsigned)((n_out + 3) / 4)), dim3(256), 0, s>>>(P.work, P.sse, n_out, P.P, P.n_fields_total);
    SEA_CHECK_LAUNCH("sea_decode_member_sse");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_member_moments: the weighted mean and the weighted, centred variance of the decoded fields over the members of each history (the forecast
// of an ensemble and its spread).  The second consumer of stage 1 above — the same W2 tiles through the same two LDS images, the same H fragments in
// registers — but it reduces over ROWS (the members of one (history, patch)) instead of over columns, so the two MFMA operands are swapped:
//   A = the H fragments: lane (li, lg) holds the hidden row of member j0 + li — rows are loaded per lane by index, so the gather
//       m = (b members + j) P + patch costs nothing,
//   B = the W2 tile from LDS, read exactly as member_sse reads its A operand (row sub 16 + li, chunk 4 ks + lg),
// and the accumulator of lane (li, lg) holds COLUMN cb + sub 16 + li for the four MEMBERS j0 + 4 lg + r.  Four members are reduced in registers, the
// four lane groups by two butterfly steps, the NW = 8 waves of a workgroup (consecutive 16-member blocks of the same (history, patch): 128 members)
// through 4 kB of LDS by the wave whose turn it is, which also stores the tile's 32 columns of both outputs.  Ensembles above 128 members run one
// workgroup per 128-member chunk, each writing its (W, mean, M2) to the workspace, and a short finish launch folds the chunks in ascending order.
//
// Numerics.  Every partial is a triple (W, mean, M2) with M2 = sum w (y - mean)^2 taken about the partial's OWN mean: a lane takes the mean of its
// (up to) four live members about the first live value, then their centred squares; partials are merged by Chan's update
//     mean = m_a + (m_b - m_a) W_b / W,   M2 = M2_a + M2_b + (m_a - m_b)^2 W_a W_b / W,   W = W_a + W_b
// in a fixed tree (lane groups (0,1),(2,3); waves ((0,1),(2,3)),((4,5),(6,7)); chunks left to right).  The weights do not depend on the column, so the
// two factors of every merge, f = W_b / W and k = W_a f, are computed once per launch and not per tile; an empty side gives f = 1, k = 0 or
// f = 0, k = 0, with which the update returns the other side's bits (an empty partial is (0, 0, 0)).  Nothing is ever formed as E[y^2] - E[y]^2.
// A member with w <= 0 (or NaN) is dead: its hidden row is not loaded, and its accumulator registers are passed over by SELECTS, so NaN or Inf in it
// reaches nothing.  A history with one live member therefore returns that member's decoded row bit for bit and a variance of exactly 0.
// Waves whose 16-member block lies beyond `members` issue no MFMAs: they help carry the W2 tiles and take their turns at the stores.
// counts: a workgroup serves ONE patch, so the column limit is uniform: only the ceil(lim / 32) tiles of a field that hold valid columns are
// fetched and multiplied; everything at or beyond them, up to ld, is zero-filled.  One writer per output element, no atomics: two runs give the same
// bits, and a history's result does not depend on the other histories of the call.
struct MemberMomentsLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeMemberMoments p;
    int n_chunks;
    float w_uniform;   // 1 / members, used when p.w == NULL
};

constexpr int MM_NW = 8;               // waves per workgroup
constexpr int MM_CHUNK = 16 * MM_NW;   // members a workgroup finishes

template <int SP>
constexpr int mm_lds_bytes() { return 2 * DM_TC * (SP * 2 + DM_PAD) + 2 * MM_NW * DM_TC * 8 + MM_NW * 4; }

// the two factors of Chan's update for partial weights Wa (left) and Wb (right)
__device__ __forceinline__ void mm_factors(float Wa, float Wb, float& f, float& k) {
    f = Wb > 0.f ? (Wa > 0.f ? Wb / (Wa + Wb) : 1.f) : 0.f;
    k = Wa * f;
}
// (ma, qa) <- merge of the left partial (ma, qa) and the right one (mb, qb)
__device__ __forceinline__ void mm_merge(float& ma, float& qa, float mb, float qb, float f, float k) {
    const float d = add1(mb, -ma);
    ma = fma1(d, f, ma);
    qa = fma1(mul1(d, d), k, add1(qa, qb));
}

template <int SP>
__global__ __launch_bounds__(64 * MM_NW) void decode_member_moments_kernel(const MemberMomentsLaunch L) {
    constexpr int NW = MM_NW;
    constexpr int NT = 64 * NW;
    constexpr int KS = SP / 32;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images; (mean, M2) of 32 columns per wave, twice; the waves' weights
    float2* red = reinterpret_cast<float2*>(smem + 2 * TILE);
    float* wsum = reinterpret_cast<float*>(smem + 2 * TILE + 2 * NW * DM_TC * 8);

    const SeaDecodeMseGroup& G = L.g[blockIdx.y];
    const SeaDecodeMemberMoments& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int S = P.S, C = P.C, Cp = P.Cp, members = P.members, ld = P.ld, nft = P.n_fields_total;
    const int n_chunks = L.n_chunks;
    const int bp = blockIdx.x / n_chunks, chunk = blockIdx.x - bp * n_chunks;
    const int b = bp / P.P, patch = bp - b * P.P;
    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    const bool last = n_chunks == 1;   // this workgroup finishes its outputs; otherwise it writes a partial per chunk

    int lim = C;   // valid columns of this patch: [0, lim) — uniform over the workgroup
    if (P.counts != nullptr) {
        const int cnt = P.counts[patch];
        lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
    }
    const int tpf = (lim + DM_TC - 1) / DM_TC;   // tiles of a field that hold valid columns
    const int64_t out0 = ((int64_t)bp * nft + G.field0) * ld;   // (bp, field0, 0) of both outputs
    if (last && tpf * DM_TC < ld) {   // columns behind the tiles: exactly 0
        const int z0 = tpf * DM_TC, zw = ld - z0;
        for (int i = tid; i < G.n_fields * zw; i += NT) {
            const int j = i / zw;
            const int64_t o = out0 + (int64_t)j * ld + z0 + (i - j * zw);
            P.mean[o] = 0.f;
            P.var[o] = 0.f;
        }
    }
    if (tpf == 0) return;   // uniform: before any barrier

    // this wave's 16-member block; the weights of the lane's four accumulator rows and of its hidden row
    const int j0 = chunk * MM_CHUNK + wave * 16;
    const bool active = j0 < members;   // uniform over the wave
    const float* wrow = P.w != nullptr ? P.w + (int64_t)b * members : nullptr;
    float wl[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int jr = j0 + 4 * lg + r;
        const float v = jr < members ? (wrow != nullptr ? wrow[jr] : L.w_uniform) : 0.f;
        wl[r] = v > 0.f ? v : 0.f;   // negative or NaN: dead
    }
    const int jm = j0 + li;
    const bool row_live = jm < members && (wrow != nullptr ? wrow[jm] : L.w_uniform) > 0.f;
    const int64_t m = ((int64_t)b * members + (jm < members ? jm : 0)) * P.P + patch;

    uint4 hf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int s = ks * 32 + 8 * lg;
        hf[ks] = (row_live && s < S) ? *reinterpret_cast<const uint4*>(H + m * G.ldh + s) : zero4;
    }

    // merge factors of the two butterfly steps (the left side is the lower lane group)
    const float Wl = add1(add1(wl[0], wl[1]), add1(wl[2], wl[3]));
    const float inv_Wl = Wl > 0.f ? 1.0f / Wl : 0.f;
    const bool left1 = (lane & 16) == 0, left2 = (lane & 32) == 0;
    float f1, k1, f2, k2;
    const float Wo1 = __shfl_xor(Wl, 16);
    mm_factors(left1 ? Wl : Wo1, left1 ? Wo1 : Wl, f1, k1);
    const float Wp = add1(left1 ? Wl : Wo1, left1 ? Wo1 : Wl);
    const float Wo2 = __shfl_xor(Wp, 32);
    mm_factors(left2 ? Wp : Wo2, left2 ? Wo2 : Wp, f2, k2);
    const float Ww = add1(left2 ? Wp : Wo2, left2 ? Wo2 : Wp);   // the wave's weight: the same bits in every lane
    if (lane == 0) wsum[wave] = Ww;
    if (!active && lane < DM_TC) {   // an empty block stays (0, 0) in both images
        red[wave * DM_TC + lane] = make_float2(0.f, 0.f);
        red[(NW + wave) * DM_TC + lane] = make_float2(0.f, 0.f);
    }

    const int n_tiles = G.n_fields * tpf;
    uint4 wr[NCH];
    dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, 0, tid);
    dm_store_tile<SP, NT>(wr, smem, tid);
    __syncthreads();

    // merge factors of the wave tree ((0,1),(2,3)),((4,5),(6,7))
    float tf[NW - 1], tk[NW - 1];
    float Wtot;
    {
        float w2[NW / 2], w4[NW / 4];
#pragma unroll
        for (int i = 0; i < NW / 2; ++i) {
            mm_factors(wsum[2 * i], wsum[2 * i + 1], tf[i], tk[i]);
            w2[i] = add1(wsum[2 * i], wsum[2 * i + 1]);
        }
#pragma unroll
        for (int i = 0; i < NW / 4; ++i) {
            mm_factors(w2[2 * i], w2[2 * i + 1], tf[NW / 2 + i], tk[NW / 2 + i]);
            w4[i] = add1(w2[2 * i], w2[2 * i + 1]);
        }
        mm_factors(w4[0], w4[1], tf[NW - 2], tk[NW - 2]);
        Wtot = add1(w4[0], w4[1]);
    }
    const int64_t n_el = (int64_t)(P.M / (P.P * members)) * P.P * nft * ld;   // elements of one output
    if (!last && G.field0 == 0 && tid == 0) P.work[2 * n_chunks * n_el + (int64_t)bp * n_chunks + chunk] = Wtot;
    const float vs = P.var_scale != nullptr ? P.var_scale[b] : 1.0f;
    float* const o_mean = P.mean;
    float* const o_var = P.var;
    float* const o_work = P.work;

    // the 32 columns of a finished tile: merge the waves' partials (lanes 0-31 and 32-63 both do), store the mean (lanes 0-31) and the variance (32-63)
    auto emit = [=](int rb, int pj, int pcb) {
        const int col = lane & 31;
        float mm[NW], qq[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const float2 v = red[(rb * NW + w) * DM_TC + col];
            mm[w] = v.x;
            qq[w] = v.y;
        }
#pragma unroll
        for (int i = 0; i < NW / 2; ++i) mm_merge(mm[2 * i], qq[2 * i], mm[2 * i + 1], qq[2 * i + 1], tf[i], tk[i]);
#pragma unroll
        for (int i = 0; i < NW / 4; ++i) mm_merge(mm[4 * i], qq[4 * i], mm[4 * i + 2], qq[4 * i + 2], tf[NW / 2 + i], tk[NW / 2 + i]);
        mm_merge(mm[0], qq[0], mm[4], qq[4], tf[NW - 2], tk[NW - 2]);
        const int c = pcb + col;
        if (c < ld) {
            const int64_t o = out0 + (int64_t)pj * ld + c;
            if (last) {
                const float v = lane < 32 ? mm[0] : mul1(qq[0], vs);
                (lane < 32 ? o_mean : o_var)[o] = c < lim ? v : 0.f;
            } else {
                o_work[(int64_t)(lane < 32 ? chunk : n_chunks + chunk) * n_el + o] = lane < 32 ? mm[0] : qq[0];
            }
        }
    };

    int j = 0, tj = 0;     // field of tile t and the tile's index inside it
    int pj = 0, pcb = 0;   // the same of tile t - 1
    for (int t = 0; t < n_tiles; ++t) {
        const char* buf = smem + (t & 1) * TILE;
        if (t + 1 < n_tiles) dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t + 1, tid);
        const int cb = tj * DM_TC;
        if (t > 0 && wave == ((t - 1) & (NW - 1))) emit((t - 1) & 1, pj, pcb);

        if (active) {
            f32x4 acc[2][2];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const float bv = G.bias[j * Cp + cb + sub * 16 + li];
                acc[sub][0] = f32x4{bv, bv, bv, bv};
                acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks * 32 < S) {
#pragma unroll
                    for (int sub = 0; sub < 2; ++sub) {
                        const uint4 wv = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                        mma16<__bf16>(hf[ks], wv, acc[sub][ks & 1]);
                    }
                }
            }
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                float y[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = acc[sub][0][r] + acc[sub][1][r];   // plain C++, as above: the first reader of an MFMA result must be an instruction the compiler sees (it places the wait states behind the MFMA; it cannot for inline assembly)
                // the lane's four members: mean about the first live value, then the centred squares; a dead member is passed over by selects
                float ref = 0.f;
#pragma unroll
                for (int r = 3; r >= 0; --r) ref = wl[r] > 0.f ? y[r] : ref;
                float sw = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) sw = wl[r] > 0.f ? fma1(wl[r], add1(y[r], -ref), sw) : sw;
                float mean = fma1(sw, inv_Wl, ref);
                float q = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = add1(y[r], -mean);
                    q = wl[r] > 0.f ? fma1(mul1(wl[r], d), d, q) : q;
                }
                // lane groups (0, 1), (2, 3), then the pairs
                float mo = __shfl_xor(mean, 16), qo = __shfl_xor(q, 16);
                float ma = left1 ? mean : mo, qa = left1 ? q : qo;
                mm_merge(ma, qa, left1 ? mo : mean, left1 ? qo : q, f1, k1);
                mo = __shfl_xor(ma, 32);
                qo = __shfl_xor(qa, 32);
                float mb = left2 ? ma : mo, qb = left2 ? qa : qo;
                mm_merge(mb, qb, left2 ? mo : ma, left2 ? qo : qa, f2, k2);
                if (lg == 0) red[((t & 1) * NW + wave) * DM_TC + sub * 16 + li] = make_float2(mb, qb);
            }
        }
        pj = j;
        pcb = cb;
        if (++tj == tpf) {
            tj = 0;
            ++j;
        }

        if (t + 1 < n_tiles) dm_store_tile<SP, NT>(wr, smem + ((t + 1) & 1) * TILE, tid);
        __syncthreads();
    }
    if (wave == ((n_tiles - 1) & (NW - 1))) emit((n_tiles - 1) & 1, pj, pcb);
}

// ensembles above 128 members: fold the chunks' partials (left to right) into the outputs; one thread per output element
__global__ __launch_bounds__(256) void member_moments_finish_kernel(const float* __restrict__ work, int n_chunks, const int32_t* __restrict__ counts,
                                                                    const float* __restrict__ var_scale, float* __restrict__ mean, float* __restrict__ var,
                                                                    int64_t n_el, int P, int nft, int ld, int C) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_el) return;
    const int c = (int)(e % ld);
    const int64_t bp = e / ld / nft;
    const int patch = (int)(bp % P);
    int lim = C;
    if (counts != nullptr) {
        const int cnt = counts[patch];
        lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
    }
    if (c >= lim) {
        mean[e] = 0.f;
        var[e] = 0.f;
        return;
    }
    const float* wm = work;
    const float* wq = work + n_chunks * n_el;
    const float* ww = work + 2 * n_chunks * n_el + bp * n_chunks;
    float W = ww[0], mu = wm[e], q = wq[e];
    for (int k = 1; k < n_chunks; ++k) {
        float f, kk;
        mm_factors(W, ww[k], f, kk);
        mm_merge(mu, q, wm[k * n_el + e], wq[k * n_el + e], f, kk);
        W = add1(W, ww[k]);
    }
    mean[e] = mu;
    var[e] = mul1(q, var_scale != nullptr ? var_scale[bp / P] : 1.0f);
}

template <int SP>
static void member_moments_launch(const MemberMomentsLaunch& L, dim3 grid, hipStream_t s) {
    constexpr int lds = mm_lds_bytes<SP>();
    static bool set_on[64] = {false};   // per device: SP = 640 needs 88 kB, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_member_moments_kernel<SP>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_member_moments_kernel<SP><<<grid, dim3(64 * MM_NW), lds, s>>>(L);
}

extern "C" int sea_decode_member_moments(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberMoments* p, int dtype, void* stream) {
    SEA_REQUIRE(groups != nullptr && p != nullptr, "sea_decode_member_moments: null argument table");
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "sea_decode_member_moments: n_groups=%d outside 1..%d", n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "sea_decode_member_moments: bad dtype %d", dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("sea_decode_member_moments: unsupported: bf16 only (the fp32 decoder composes sea_gemm_grouped and reductions)");
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeMemberMoments& P = *p;
    SEA_REQUIRE(P.mean != nullptr && P.var != nullptr, "sea_decode_member_moments: null mean or var pointer");
    SEA_REQUIRE(P.M >= 1, "sea_decode_member_moments: M=%d must be positive", P.M);
    SEA_REQUIRE(P.S >= 8 && P.S % 8 == 0, "sea_decode_member_moments: S=%d must be a positive multiple of 8", P.S);
    SEA_REQUIRE(P.Cp >= 32 && P.Cp % 32 == 0, "sea_decode_member_moments: Cp=%d must be a positive multiple of 32", P.Cp);
    SEA_REQUIRE(P.C >= 1 && P.C <= P.Cp, "sea_decode_member_moments: C=%d must lie in 1..Cp=%d", P.C, P.Cp);
    SEA_REQUIRE(P.P >= 1 && P.members >= 1, "sea_decode_member_moments: P=%d and members=%d must be positive", P.P, P.members);
    SEA_REQUIRE((int64_t)P.M % ((int64_t)P.P * P.members) == 0, "sea_decode_member_moments: M=%d is not a multiple of P * members = %d * %d", P.M, P.P, P.members);
    SEA_REQUIRE(P.n_fields_total >= 1, "sea_decode_member_moments: n_fields_total=%d must be positive", P.n_fields_total);
    SEA_REQUIRE(P.ld >= P.C && P.ld % 4 == 0, "sea_decode_member_moments: output row stride ld=%d must cover C=%d and be a multiple of 4", P.ld, P.C);
    SEA_REQUIRE(sea_aligned16(P.mean) && sea_aligned16(P.var) && sea_aligned4(P.w) && sea_aligned4(P.var_scale) && sea_aligned4(P.counts) && sea_aligned4(P.work),
                "sea_decode_member_moments: misaligned mean, var (16 bytes), w, var_scale, counts or work (4 bytes) pointer");
    int64_t covered = 0;
    for (int g = 0; g < n_groups; ++g) {
        const SeaDecodeMseGroup& G = groups[g];
        SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr, "sea_decode_member_moments: group %d: null pointer", g);
        SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias), "sea_decode_member_moments: group %d: pointers must be 16-byte aligned", g);
        SEA_REQUIRE(G.ldh >= P.S && G.ldh % 8 == 0 && G.ldw >= P.S && G.ldw % 8 == 0,
                    "sea_decode_member_moments: group %d: row strides ldh=%d ldw=%d must cover S=%d and be multiples of 8", g, G.ldh, G.ldw, P.S);
        SEA_REQUIRE(G.n_fields >= 1 && G.field0 >= 0 && (int64_t)G.field0 + G.n_fields <= P.n_fields_total,
                    "sea_decode_member_moments: group %d: n_fields=%d, field0=%d outside the %d fields", g, G.n_fields, G.field0, P.n_fields_total);
        SEA_REQUIRE((int64_t)G.n_fields * P.Cp <= 0x7fffffffLL / 2, "sea_decode_member_moments: group %d: too many output columns", g);
        for (int h = 0; h < g; ++h)
            SEA_REQUIRE(G.field0 >= groups[h].field0 + groups[h].n_fields || groups[h].field0 >= G.field0 + G.n_fields,
                        "sea_decode_member_moments: group %d: its fields overlap those of group %d (every output element has one writer)", g, h);
        covered += G.n_fields;
    }
    SEA_REQUIRE(covered == P.n_fields_total, "sea_decode_member_moments: the groups cover %lld of the %d fields (every field needs exactly one group)", (long long)covered, P.n_fields_total);
    if (P.S > 640) {
        sea_set_error("sea_decode_member_moments: unsupported: hidden width S=%d above 640", P.S);
        return SEA_EUNSUPPORTED;
    }
    const int64_t BP = (int64_t)P.M / P.members;   // (history, patch) pairs: rows of the outputs
    const int64_t n_chunks = ((int64_t)P.members + MM_CHUNK - 1) / MM_CHUNK;
    const int64_t n_el = BP * P.n_fields_total * P.ld;
    SEA_REQUIRE(BP * n_chunks <= 0x7fffffffLL && (n_el + 255) / 256 <= 0x7fffffffLL, "sea_decode_member_moments: too many rows");
    if (n_chunks > 1) {
        const int64_t need = n_chunks * (2 * n_el + BP);
        SEA_REQUIRE(P.work != nullptr && P.work_cap >= need,
                    "sea_decode_member_moments: workspace of %lld floats is too small: %lld needed (ceil(members / 128) * (2 * outputs + M / members); members=%d above 128)",
                    (long long)(P.work != nullptr ? P.work_cap : 0), (long long)need, P.members);
    }

    MemberMomentsLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    L.n_chunks = (int)n_chunks;
    L.w_uniform = 1.0f / (float)P.members;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(BP * n_chunks), (unsigned)n_groups);
    if (P.S <= 128) member_moments_launch<128>(L, grid, s);
    else if (P.S <= 256) member_moments_launch<256>(L, grid, s);
    else if (P.S <= 384) member_moments_launch<384>(L, grid, s);
    else if (P.S <= 512) member_moments_launch<512>(L, grid, s);
    else member_moments_launch<640>(L, grid, s);
    if (n_chunks > 1)
        member_moments_finish_kernel<<<dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, s>>>(P.work, (int)n_chunks, P.counts, P.var_scale, P.mean, P.var, n_el, P.P,
                                                                                                   P.n_fields_total, P.ld, P.C);
    SEA_CHECK_LAUNCH("sea_decode_member_moments");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_sensor_sse: the precision-weighted squared error of every ensemble member against SPARSE observations — K sensors, each reading one
// decoded field at one cell of one patch (ensemble weighting from probes instead of a dense snapshot).  Stage 1 of decode_mse_kernel once more, with
// two changes: the 32 W2 rows of a tile are GATHERED through an index table (wrow: the sensors of one (group, patch) segment, sorted and padded to a
// multiple of 32 by the host), and the other operand holds only the hidden rows of the observed patches (H is patch-major: row q Bm + bm is member bm
// at observed patch q).  Workgroup (x, y, z) serves the 64-member row tile x of observed patch y and group z; wave w the members 16 w .. 16 w + 15; a
// lane holds one member (lane & 15) and 8 of a tile's 32 sensors (sorted positions 16 sub + 4 (lane >> 4) + r), as in decode_member_sse_kernel.  A
// (group, patch) pair without sensors is an empty segment: its workgroup writes zeros and leaves before any barrier.
// Epilogue, per sensor: w = live and prec > 0 ? prec : 0; d = w > 0 ? y - obs : 0 (selects: a sensor without weight is neutral whatever obs holds, NaN
// and Inf included); sum += (w d) d in fp32.  The lane adds its 8 sensors per tile over the tiles in order, the four lanes of a member are folded by
// two butterfly steps, lane group 0 writes work[(y G + z) Bm + bm]: one writer per element, no atomics.  sensor_sse_finish_kernel adds a member's Q G
// partials in ascending order.  A 16-row tile may straddle histories, so every lane derives its own history b = bm / members for obs and prec.  A
// member's arithmetic touches nothing of the other rows of its tile (an MFMA column is a dot product of its own operands), so its score does not
// depend on the tile it falls into, on `members` or on the number of histories: the same bits.  With pred != NULL the decoded values are stored
// too, at pred[bm K_pad + sorted position] (pad positions included: their W2 row is row 0 — a defined value the caller drops).
// The kernel trusts wrow (rows of W2) and seg: the host builds and range-checks them (sea_amd/ensemble.py, SensorSet).
struct SensorSseLaunch {
    static constexpr bool derived = false;
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeSensorSse p;
};
// The same launch with the pair tables of sea_decode_derived_sensor_sse behind it (the kernels below are compiled once per launch type; everything
// the derived form adds sits in `if constexpr (LT::derived)`, so the plain form's code is what it was).
struct DerivedSensorSseLaunch {
    static constexpr bool derived = true;
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeSensorSse p;
    SeaDerivedSensorTables t;
};
__device__ __forceinline__ float dv_value(const int op, const float ya, const float yb, const float sa, const float ha, const float sb, const float hb);   // below

// A lane's 4 consecutive sorted positions are two PAIRS (2 i, 2 i + 1) = (source a, source b) of one reading: x of pair pr from the decoded values, in
// registers.  op < 0: a plain reading, x = ya.  Both entries of y get x (pred[2 i] = pred[2 i + 1] = x).
__device__ __forceinline__ float ds_pair_value(const int op, const float ya, const float yb, const float sa, const float ha, const float sb, const float hb) {
    const float x = dv_value(op < 0 ? SEA_DERIVED_DIFFERENCE : op, ya, yb, sa, ha, sb, hb);
    return op < 0 ? ya : x;
}

// dm_load_tile with gathered rows: row i of the tile is W2 row rows[i]; the 16-byte chunks of a row stay contiguous
template <int SP, int NT = 256>
__device__ __forceinline__ void ds_load_tile_gathered(uint4 (&wr)[SP * 4 / NT], const __bf16* W2, int ldw, int S, const int32_t* __restrict__ rows, int tid) {
    constexpr int CPR = SP / 8;
#pragma unroll
    for (int u = 0; u < SP * 4 / NT; ++u) {
        const int q = u * NT + tid, r = q / CPR, ch = q - r * CPR;
        wr[u] = ch * 8 < S ? *reinterpret_cast<const uint4*>(W2 + (int64_t)rows[r] * ldw + ch * 8) : make_uint4(0u, 0u, 0u, 0u);
    }
}

template <int SP, class LT = SensorSseLaunch>
__global__ __launch_bounds__(256) void decode_sensor_sse_kernel(const LT L) {
#pragma clang fp reassociate(off)   // the lane's sum runs over its sensors in the stated order
    constexpr int NT = 256;
    constexpr int KS = SP / 32;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images

    const SeaDecodeMseGroup& G = L.g[blockIdx.z];
    const SeaDecodeSensorSse& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int Bm = P.Bm, S = P.S;
    const int q = blockIdx.y, n_g = gridDim.z;
    const int bm = blockIdx.x * DM_ROWS + wave * 16 + li;   // the member this lane holds
    float* const wslot = P.work + ((int64_t)q * n_g + blockIdx.z) * Bm + (bm < Bm ? bm : 0);

    const int seg0 = P.seg[(int64_t)blockIdx.z * (P.Q + 1) + q], seg1 = P.seg[(int64_t)blockIdx.z * (P.Q + 1) + q + 1];
    const int n_tiles = (seg1 - seg0) / DM_TC;
    if (n_tiles <= 0) {   // uniform over the workgroup, before any barrier: no sensor of this group in this patch
        if (lg == 0 && bm < Bm) *wslot = 0.f;
        return;
    }

    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    uint4 hf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int s = ks * 32 + 8 * lg;
        hf[ks] = (bm < Bm && s < S) ? *reinterpret_cast<const uint4*>(H + ((int64_t)q * Bm + bm) * G.ldh + s) : zero4;
    }
    const int b = bm < Bm ? bm / P.members : 0;   // the lane's history: a row beyond Bm reads history 0 and stores nothing
    const float* orow = P.obs + (int64_t)b * P.ld_obs;
    const float* prow = P.prec != nullptr ? P.prec + (int64_t)b * P.ld_prec : nullptr;
    float* drow = P.pred != nullptr && bm < Bm ? P.pred + (int64_t)bm * P.K_pad : nullptr;

    uint4 wr[NCH];
    ds_load_tile_gathered<SP, NT>(wr, W2, G.ldw, S, P.wrow + seg0, tid);
    dm_store_tile<SP, NT>(wr, smem, tid);
    __syncthreads();

    float fsum = 0.f;
    for (int t = 0; t < n_tiles; ++t) {
        const char* buf = smem + (t & 1) * TILE;
        const int k0 = seg0 + t * DM_TC;   // sorted position of the tile's first sensor
        if (t + 1 < n_tiles) ds_load_tile_gathered<SP, NT>(wr, W2, G.ldw, S, P.wrow + k0 + DM_TC, tid);

        // observation, precision and the live mask of this lane's 2 x 4 sensors (requested now, used after the products); the bias through the row table
        float ob[2][4], pw[2][4];
        f32x4 acc[2][2];
        [[maybe_unused]] int4 dop[2];
        [[maybe_unused]] float4 dsc[2], dsh[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int k = k0 + sub * 16 + 4 * lg;   // a multiple of 4: obs, prec and pred rows start 16-byte aligned (K_pad % 32 == 0, strides % 4 == 0)
            const float4 o = *reinterpret_cast<const float4*>(orow + k);
            ob[sub][0] = o.x; ob[sub][1] = o.y; ob[sub][2] = o.z; ob[sub][3] = o.w;
            float4 pv = make_float4(1.f, 1.f, 1.f, 1.f);
            if (prow != nullptr) pv = *reinterpret_cast<const float4*>(prow + k);
            pw[sub][0] = pv.x; pw[sub][1] = pv.y; pw[sub][2] = pv.z; pw[sub][3] = pv.w;
            f32x4 bv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pw[sub][r] = (P.live[k + r] != 0 && pw[sub][r] > 0.f) ? pw[sub][r] : 0.f;   // pad entries, zero, negative and NaN precisions: no weight
                bv[r] = G.bias[P.wrow[k + r]];
            }
            acc[sub][0] = bv;
            acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (LT::derived) {   // the pair tables of this lane's two pairs, as obs and prec: one 16-byte load each
                dop[sub] = *reinterpret_cast<const int4*>(L.t.op + k);
                dsc[sub] = *reinterpret_cast<const float4*>(L.t.scale + k);
                dsh[sub] = *reinterpret_cast<const float4*>(L.t.shift + k);
            }
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks * 32 < S) {
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    const uint4 a = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                    mma16<__bf16>(a, hf[ks], acc[sub][ks & 1]);
                }
            }
        }

#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            float y[4];
            if constexpr (LT::derived) {
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = acc[sub][0][r] + acc[sub][1][r];   // sea_decode_sensor_sse's y: the same accumulators, the same bits
                const float x0 = ds_pair_value(dop[sub].x, y[0], y[1], dsc[sub].x, dsh[sub].x, dsc[sub].y, dsh[sub].y);
                const float x1 = ds_pair_value(dop[sub].z, y[2], y[3], dsc[sub].z, dsh[sub].z, dsc[sub].w, dsh[sub].w);
                y[0] = y[1] = x0;
                y[2] = y[3] = x1;
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {   // the weight, the observation and the residual of a pair are those of its entry 2 i
                    const float w = pw[sub][2 * pr];
                    const float d = w > 0.f ? y[2 * pr] - ob[sub][2 * pr] : 0.f;
                    fsum = __builtin_fmaf(w * d, d, fsum);
                }
            } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                y[r] = acc[sub][0][r] + acc[sub][1][r];
                const float w = pw[sub][r];
                const float d = w > 0.f ? y[r] - ob[sub][r] : 0.f;
                fsum = __builtin_fmaf(w * d, d, fsum);
            }
            }
            if (drow != nullptr) *reinterpret_cast<float4*>(drow + k0 + sub * 16 + 4 * lg) = make_float4(y[0], y[1], y[2], y[3]);
        }

        if (t + 1 < n_tiles) dm_store_tile<SP, NT>(wr, smem + ((t + 1) & 1) * TILE, tid);
        __syncthreads();
    }

    // fold the member's four lanes, one writer
    float v = fsum;
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lg == 0 && bm < Bm) *wslot = v;
}

// wsse[bm] = sum of the member's Q * G partials work[i Bm + bm], i ascending: a fixed order
__global__ __launch_bounds__(256) void sensor_sse_finish_kernel(const float* __restrict__ work, float* __restrict__ wsse, int Bm, int n_part) {
#pragma clang fp reassociate(off)   // the order IS the contract: with the file's -ffast-math the loop was vectorised into two partial sums when Bm == 1 — other bits than at Bm > 1
    const int bm = blockIdx.x * 256 + threadIdx.x;
    if (bm >= Bm) return;
    float acc = 0.f;
    for (int i = 0; i < n_part; ++i) acc += work[(int64_t)i * Bm + bm];
    wsse[bm] = acc;
}

template <int SP, class LT>
static void sensor_sse_launch(const LT& L, dim3 grid, hipStream_t s) {
    constexpr int lds = 2 * DM_TC * (SP * 2 + DM_PAD);
    static bool set_on[64] = {false};   // per device (and per launch type): SP = 640 needs 84 kB, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_sensor_sse_kernel<SP, LT>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_sensor_sse_kernel<SP, LT><<<grid, dim3(256), lds, s>>>(L);
}

// The checks the four sensor entry points share, under the entry point's name `who`.  P: the fields SeaDecodeSensorGrad has in common with
// SeaDecodeSensorSse; grad_scale: NULL for the score-only entry points; derived: the pair tables are required (t) — the plain entry points pass
// false and NULL; composes: what the message of the unsupported fp32 form names as the caller's other path.  SEA_OK, SEA_EINVAL or SEA_EUNSUPPORTED.
static int sensor_args_check(const char* who, const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeSensorSse& P, const float* grad_scale, bool derived,
                             const SeaDerivedSensorTables* t, int dtype, const char* composes) {
    const bool grad = grad_scale != nullptr;
    SEA_REQUIRE(groups != nullptr && (!derived || t != nullptr), "%s: null argument table", who);
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "%s: n_groups=%d outside 1..%d", who, n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "%s: bad dtype %d", who, dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("%s: unsupported: bf16 only (the fp32 decoder composes %s)", who, composes);
        return SEA_EUNSUPPORTED;
    }
    SEA_REQUIRE(P.obs != nullptr && P.live != nullptr && P.wrow != nullptr && P.seg != nullptr && P.wsse != nullptr && P.work != nullptr,
                "%s: null obs, live, wrow, seg, wsse or work pointer", who);
    SEA_REQUIRE(!derived || (t->op != nullptr && t->scale != nullptr && t->shift != nullptr), "%s: null op, scale or shift table", who);
    SEA_REQUIRE(P.Bm >= 1 && P.members >= 1 && P.Bm % P.members == 0, "%s: Bm=%d must be a positive multiple of members=%d", who, P.Bm, P.members);
    SEA_REQUIRE(P.S >= 8 && P.S % 8 == 0, "%s: S=%d must be a positive multiple of 8", who, P.S);
    SEA_REQUIRE(P.Cp >= 32 && P.Cp % 32 == 0, "%s: Cp=%d must be a positive multiple of 32", who, P.Cp);
    SEA_REQUIRE(P.K_pad >= 32 && P.K_pad % 32 == 0, "%s: K_pad=%d must be a positive multiple of 32", who, P.K_pad);
    SEA_REQUIRE(P.Q >= 1 && P.Q <= 65535, "%s: Q=%d observed patches outside 1..65535", who, P.Q);
    SEA_REQUIRE(P.ld_obs >= P.K_pad && P.ld_obs % 4 == 0, "%s: obs row stride ld_obs=%lld must cover K_pad=%d and be a multiple of 4", who, (long long)P.ld_obs, P.K_pad);
    SEA_REQUIRE(P.prec == nullptr || P.ld_prec == 0 || (P.ld_prec >= P.K_pad && P.ld_prec % 4 == 0),
                "%s: prec row stride ld_prec=%lld must be 0 (one row for all histories) or cover K_pad=%d and be a multiple of 4", who, (long long)P.ld_prec, P.K_pad);
    SEA_REQUIRE(sea_aligned16(P.obs) && sea_aligned16(P.prec) && sea_aligned16(P.pred), "%s: obs, prec and pred must be 16-byte aligned", who);
    SEA_REQUIRE(sea_aligned4(P.live) && sea_aligned4(P.wrow) && sea_aligned4(P.seg) && sea_aligned4(P.wsse) && sea_aligned4(P.work),
                "%s: misaligned live, wrow, seg, wsse or work pointer", who);
    SEA_REQUIRE(!derived || (sea_aligned16(t->op) && sea_aligned16(t->scale) && sea_aligned16(t->shift)), "%s: the op, scale and shift tables must be 16-byte aligned", who);
    if (grad) {
        uint32_t gs_bits;
        memcpy(&gs_bits, grad_scale, sizeof(gs_bits));
        SEA_REQUIRE((gs_bits & 0x7f800000u) != 0x7f800000u, "%s: grad_scale must be finite", who);   // the exponent field itself: no floating-point compare to reason about
    }
    for (int g = 0; g < n_groups; ++g) {
        const SeaDecodeMseGroup& G = groups[g];
        if (!grad) {
            SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr, "%s: group %d: null pointer", who, g);
            SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias), "%s: group %d: pointers must be 16-byte aligned", who, g);
        } else {
            SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr && G.dH != nullptr, "%s: group %d: null pointer (H, W2, bias or dH)", who, g);
            SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias) && sea_aligned16(G.dH) && sea_aligned16(G.Z),
                        "%s: group %d: pointers must be 16-byte aligned", who, g);
        }
        SEA_REQUIRE(G.ldh >= P.S && G.ldh % 8 == 0 && G.ldw >= P.S && G.ldw % 8 == 0, "%s: group %d: row strides ldh=%d ldw=%d must cover S=%d and be multiples of 8", who,
                    g, G.ldh, G.ldw, P.S);
        if (grad)
            SEA_REQUIRE(G.lddh >= P.S && G.lddh % 8 == 0 && (G.Z == nullptr || (G.ldz >= P.S && G.ldz % 8 == 0)),
                        "%s: group %d: row strides lddh=%d ldz=%d must cover S=%d and be multiples of 8", who, g, G.lddh, G.ldz, P.S);
        SEA_REQUIRE(G.n_fields >= 1 && (int64_t)G.n_fields * P.Cp <= 0x7fffffffLL / 2, "%s: group %d: n_fields=%d", who, g, G.n_fields);
    }
    if (P.S > 640) {
        sea_set_error("%s: unsupported: hidden width S=%d above 640", who, P.S);
        return SEA_EUNSUPPORTED;
    }
    const int64_t row_blocks = ((int64_t)P.Bm + DM_ROWS - 1) / DM_ROWS;
    const int64_t need = (int64_t)P.Q * n_groups * P.Bm;
    SEA_REQUIRE(row_blocks <= 0x7fffffffLL && (int64_t)P.Q * P.Bm <= 0x7fffffffLL, "%s: too many rows", who);
    SEA_REQUIRE(P.work_cap >= need, "%s: workspace of %lld floats is too small: %lld needed (Q * n_groups * Bm)", who, (long long)P.work_cap, (long long)need);
    return SEA_OK;
}

// The fields SeaDecodeSensorGrad has in common with SeaDecodeSensorSse, for the shared checks.
static SeaDecodeSensorSse sensor_common(const SeaDecodeSensorGrad& P) {
    SeaDecodeSensorSse c;
    c.obs = P.obs; c.prec = P.prec; c.live = P.live; c.wrow = P.wrow; c.seg = P.seg; c.wsse = P.wsse; c.pred = P.pred; c.work = P.work;
    c.ld_obs = P.ld_obs; c.ld_prec = P.ld_prec; c.work_cap = P.work_cap;
    c.Bm = P.Bm; c.members = P.members; c.S = P.S; c.Cp = P.Cp; c.Q = P.Q; c.K_pad = P.K_pad;
    return c;
}

extern "C" int sea_decode_sensor_sse(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeSensorSse* p, int dtype, void* stream) {
    SEA_REQUIRE(groups != nullptr && p != nullptr, "sea_decode_sensor_sse: null argument table");
    const SeaDecodeSensorSse& P = *p;
    const int rc = sensor_args_check("sea_decode_sensor_sse", groups, n_groups, P, nullptr, false, nullptr, dtype, "sea_gemm_grouped, a gather and reductions");
    if (rc != SEA_OK) return rc;
    const int64_t row_blocks = ((int64_t)P.Bm + DM_ROWS - 1) / DM_ROWS;

    SensorSseLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)row_blocks, (unsigned)P.Q, (unsigned)n_groups);
    if (P.S <= 128) sensor_sse_launch<128>(L, grid, s);
    else if (P.S <= 256) sensor_sse_launch<256>(L, grid, s);
    else if (P.S <= 384) sensor_sse_launch<384>(L, grid, s);
    else if (P.S <= 512) sensor_sse_launch<512>(L, grid, s);
    else sensor_sse_launch<640>(L, grid, s);
    sea_note_form("sensor_sse.rows64", 0, 0);
    sensor_sse_finish_kernel<<<dim3((unsigned)((P.Bm + 255) / 256)), dim3(256), 0, s>>>(P.work, P.wsse, P.Bm, (int)((int64_t)P.Q * n_groups));
    SEA_CHECK_LAUNCH("sea_decode_sensor_sse");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_sensor_grad: the sparse-sensor score WITH its gradient to the hidden rows of the observed patches — decode_sensor_sse_kernel (gathered W2
// tiles, patch-major hidden rows, precision-weighted epilogue) crossed with the second MFMA stage of decode_mse_kernel.  The workgroup, the waves, the
// H fragments, the two LDS images [32][SP] with the pitch of 2 SP + 32 bytes, the prefetch of tile t + 1 before the MFMAs of tile t and the one barrier
// per tile are those of the two parents.  Per tile and wave:
//   stage 1  exactly decode_sensor_sse_kernel's: the same accumulators (bias through the row table, even / odd k-steps), the same per-lane order of the
//            sum, the same butterfly, the same work slot and the same finish launch — wsse and pred are that kernel's bits,
//   between  r = bf16(w d), rounded ONCE: the lane's 2 x 4 weighted residuals are the A fragment of stage 2 with k-slot (g, j) = tile row 4 g + j or
//            16 + 4 g + j - 4, as in decode_mse_kernel (a sensor without weight has w d = 0 by the select: its W2 row is multiplied by an exact zero),
//   stage 2  dH[bm, s] += sum_k r[bm, k] W2[wrow[k], s]: the SAME gathered image read column-wise (two ds_read_b64_tr_b16 per 16 hidden columns).
// A wave carries SP / 8 fragment registers and SP / 4 fp32 dH accumulators per lane, the budget of decode_mse_kernel (one wave per SIMD at SP = 640).
// The tiles of a segment are accumulated in ascending order into registers and stored once: dH row q Bm + bm, columns [0, S), has one writer; the
// workgroup of an EMPTY segment stores zeros there (and its zero partial) and then leaves, before any barrier.  A row of an MFMA result depends on its
// own operand row only, so a member's dH rows and score do not depend on `members`, on the number of histories or on the row tile it falls into.
// The kernel trusts wrow and seg exactly as decode_sensor_sse_kernel does.
struct SensorGradLaunch {
    static constexpr bool derived = false;
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeSensorGrad p;
};
struct DerivedSensorGradLaunch {
    static constexpr bool derived = true;
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeSensorGrad p;
    SeaDerivedSensorTables t;
};

// ds_pair_value with the two partial derivatives ga = dx / dya, gb = dx / dyb, in fp32 from the same a', b' and x (include/sea_hip.h states the table;
// single instructions, so that nothing is packed or contracted): plain 1, 0; difference sa, -sb; energy a' sa, b' sb; magnitude a' sa / x, b' sb / x
// by a select that gives exactly 0 at x = 0.
__device__ __forceinline__ float ds_pair_grad(const int op, const float ya, const float yb, const float sa, const float ha, const float sb, const float hb, float& ga,
                                              float& gb) {
    const float x = ds_pair_value(op, ya, yb, sa, ha, sb, hb);
    const float a = add1(mul1(ya, sa), ha), b = add1(mul1(yb, sb), hb);   // dv_value's a', b': the same two instructions each, the same bits
    const float as = mul1(a, sa), bs = mul1(b, sb);
    const float rx = __builtin_amdgcn_rcpf(x);
    const float ma = x > 0.f ? mul1(as, rx) : 0.f, mb = x > 0.f ? mul1(bs, rx) : 0.f;
    ga = op < 0 ? 1.f : op == SEA_DERIVED_DIFFERENCE ? sa : op == SEA_DERIVED_ENERGY ? as : ma;
    gb = op < 0 ? 0.f : op == SEA_DERIVED_DIFFERENCE ? -sb : op == SEA_DERIVED_ENERGY ? bs : mb;
    return x;
}

template <int SP, class LT = SensorGradLaunch>
__global__ __launch_bounds__(256) void decode_sensor_grad_kernel(const LT L) {
#pragma clang fp reassociate(off)   // the lane's sum runs over its sensors in the stated order
    constexpr int NT = 256;
    constexpr int KS = SP / 32;
    constexpr int ST = SP / 16;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images

    const SeaDecodeMseGroup& G = L.g[blockIdx.z];
    const SeaDecodeSensorGrad& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int Bm = P.Bm, S = P.S;
    const int q = blockIdx.y, n_g = gridDim.z;
    const int row0 = blockIdx.x * DM_ROWS + wave * 16;
    const int bm = row0 + li;   // the member this lane holds in the H fragments, in the stage-1 result and in the residual fragment
    float* const wslot = P.work + ((int64_t)q * n_g + blockIdx.z) * Bm + (bm < Bm ? bm : 0);
    __bf16* dH = static_cast<__bf16*>(G.dH);

    const int seg0 = P.seg[(int64_t)blockIdx.z * (P.Q + 1) + q], seg1 = P.seg[(int64_t)blockIdx.z * (P.Q + 1) + q + 1];
    const int n_tiles = (seg1 - seg0) / DM_TC;
    if (n_tiles <= 0) {   // uniform over the workgroup, before any barrier: no sensor of this group in this patch — zero rows, a zero partial
        if (lg == 0 && bm < Bm) *wslot = 0.f;
        const int mrows = Bm - blockIdx.x * DM_ROWS < DM_ROWS ? Bm - blockIdx.x * DM_ROWS : DM_ROWS;
        const int cpr = S / 8;   // 16-byte chunks of a row (S % 8 == 0, lddh % 8 == 0, dH 16-byte aligned)
        for (int i = tid; i < mrows * cpr; i += NT) {
            const int r = i / cpr, ch = i - r * cpr;
            *reinterpret_cast<uint4*>(dH + ((int64_t)q * Bm + blockIdx.x * DM_ROWS + r) * G.lddh + ch * 8) = make_uint4(0u, 0u, 0u, 0u);
        }
        return;
    }

    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
    uint4 hf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int s = ks * 32 + 8 * lg;
        hf[ks] = (bm < Bm && s < S) ? *reinterpret_cast<const uint4*>(H + ((int64_t)q * Bm + bm) * G.ldh + s) : zero4;
    }
    f32x4 dh[ST];
#pragma unroll
    for (int st = 0; st < ST; ++st) dh[st] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int b = bm < Bm ? bm / P.members : 0;   // the lane's history: a row beyond Bm reads history 0 and stores nothing
    const float* orow = P.obs + (int64_t)b * P.ld_obs;
    const float* prow = P.prec != nullptr ? P.prec + (int64_t)b * P.ld_prec : nullptr;
    float* drow = P.pred != nullptr && bm < Bm ? P.pred + (int64_t)bm * P.K_pad : nullptr;

    uint4 wr[NCH];
    ds_load_tile_gathered<SP, NT>(wr, W2, G.ldw, S, P.wrow + seg0, tid);
    dm_store_tile<SP, NT>(wr, smem, tid);
    __syncthreads();

    float fsum = 0.f;
    typedef dm_s16x4 __attribute__((address_space(3))) * lds_p;
    for (int t = 0; t < n_tiles; ++t) {
        const char* buf = smem + (t & 1) * TILE;
        const int k0 = seg0 + t * DM_TC;   // sorted position of the tile's first sensor
        if (t + 1 < n_tiles) ds_load_tile_gathered<SP, NT>(wr, W2, G.ldw, S, P.wrow + k0 + DM_TC, tid);

        // stage 1, as decode_sensor_sse_kernel
        float ob[2][4], pw[2][4];
        f32x4 acc[2][2];
        [[maybe_unused]] int4 dop[2];
        [[maybe_unused]] float4 dsc[2], dsh[2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int k = k0 + sub * 16 + 4 * lg;
            const float4 o = *reinterpret_cast<const float4*>(orow + k);
            ob[sub][0] = o.x; ob[sub][1] = o.y; ob[sub][2] = o.z; ob[sub][3] = o.w;
            float4 pv = make_float4(1.f, 1.f, 1.f, 1.f);
            if (prow != nullptr) pv = *reinterpret_cast<const float4*>(prow + k);
            pw[sub][0] = pv.x; pw[sub][1] = pv.y; pw[sub][2] = pv.z; pw[sub][3] = pv.w;
            f32x4 bv;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pw[sub][r] = (P.live[k + r] != 0 && pw[sub][r] > 0.f) ? pw[sub][r] : 0.f;
                bv[r] = G.bias[P.wrow[k + r]];
            }
            acc[sub][0] = bv;
            acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (LT::derived) {   // the pair tables of this lane's two pairs, as obs and prec: one 16-byte load each
                dop[sub] = *reinterpret_cast<const int4*>(L.t.op + k);
                dsc[sub] = *reinterpret_cast<const float4*>(L.t.scale + k);
                dsh[sub] = *reinterpret_cast<const float4*>(L.t.shift + k);
            }
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks * 32 < S) {
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    const uint4 a = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                    mma16<__bf16>(a, hf[ks], acc[sub][ks & 1]);
                }
            }
        }

        // score, predictions, and the weighted residual rounded once
        bf16x8 dfr;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            float y[4];
            if constexpr (LT::derived) {
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = acc[sub][0][r] + acc[sub][1][r];
                float gr[4];
                const float x0 = ds_pair_grad(dop[sub].x, y[0], y[1], dsc[sub].x, dsh[sub].x, dsc[sub].y, dsh[sub].y, gr[0], gr[1]);
                const float x1 = ds_pair_grad(dop[sub].z, y[2], y[3], dsc[sub].z, dsh[sub].z, dsc[sub].w, dsh[sub].w, gr[2], gr[3]);
                y[0] = y[1] = x0;
                y[2] = y[3] = x1;
#pragma unroll
                for (int pr = 0; pr < 2; ++pr) {   // the score of sea_decode_derived_sensor_sse; r[2 i] = act(w d ga), r[2 i + 1] = act(w d gb)
                    const float w = pw[sub][2 * pr];
                    const float d = w > 0.f ? y[2 * pr] - ob[sub][2 * pr] : 0.f;
                    const float wd = w * d;
                    fsum = __builtin_fmaf(wd, d, fsum);
                    dfr[sub * 4 + 2 * pr] = (__bf16)mul1(wd, gr[2 * pr]);
                    dfr[sub * 4 + 2 * pr + 1] = (__bf16)mul1(wd, gr[2 * pr + 1]);
                }
            } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                y[r] = acc[sub][0][r] + acc[sub][1][r];
                const float w = pw[sub][r];
                const float d = w > 0.f ? y[r] - ob[sub][r] : 0.f;
                const float wd = w * d;
                fsum = __builtin_fmaf(wd, d, fsum);
                dfr[sub * 4 + r] = (__bf16)wd;
            }
            }
            if (drow != nullptr) *reinterpret_cast<float4*>(drow + k0 + sub * 16 + 4 * lg) = make_float4(y[0], y[1], y[2], y[3]);
        }
        const uint4 da = __builtin_bit_cast(uint4, dfr);

        // stage 2, as decode_mse_kernel
        const char* tb = buf + (4 * lg + (li >> 2)) * PITCH + (4 * (li & 3)) * 2;
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            if (st * 16 < S) {
                const dm_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(tb + st * 32));
                const dm_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(tb + st * 32 + 16 * PITCH));
                const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                mma16<__bf16>(da, make_uint4(l2.x, l2.y, h2.x, h2.y), dh[st]);
            }
        }

        if (t + 1 < n_tiles) dm_store_tile<SP, NT>(wr, smem + ((t + 1) & 1) * TILE, tid);
        __syncthreads();
    }

    // dH: register r of tile st is member row0 + 4 g + r, column 16 st + (lane & 15)
    const float scale = 2.0f * P.grad_scale;
    const __bf16* Z = static_cast<const __bf16*>(G.Z);
#pragma unroll
    for (int st = 0; st < ST; ++st) {
        const int s = st * 16 + li;
        if (s < S) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int mr = row0 + 4 * lg + r;
                if (mr < Bm) {
                    const int64_t row = (int64_t)q * Bm + mr;
                    float v = dh[st][r] * scale;
                    if (Z != nullptr) v *= gelu_grad_for<__bf16>((float)Z[row * G.ldz + s]);
                    dH[row * G.lddh + s] = (__bf16)v;
                }
            }
        }
    }

    // fold the member's four lanes, one writer
    float v = fsum;
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lg == 0 && bm < Bm) *wslot = v;
}

template <int SP, class LT>
static void sensor_grad_launch(const LT& L, dim3 grid, hipStream_t s) {
    constexpr int lds = 2 * DM_TC * (SP * 2 + DM_PAD);
    static bool set_on[64] = {false};   // per device (and per launch type): SP = 640 needs 84 kB, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_sensor_grad_kernel<SP, LT>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_sensor_grad_kernel<SP, LT><<<grid, dim3(256), lds, s>>>(L);
}

extern "C" int sea_decode_sensor_grad(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeSensorGrad* p, int dtype, void* stream) {
    SEA_REQUIRE(groups != nullptr && p != nullptr, "sea_decode_sensor_grad: null argument table");
    const SeaDecodeSensorGrad& P = *p;
    const int rc = sensor_args_check("sea_decode_sensor_grad", groups, n_groups, sensor_common(P), &P.grad_scale, false, nullptr, dtype,
                                     "sea_gemm_grouped, a gather and reductions under autograd");
    if (rc != SEA_OK) return rc;
    const int64_t row_blocks = ((int64_t)P.Bm + DM_ROWS - 1) / DM_ROWS;

    SensorGradLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)row_blocks, (unsigned)P.Q, (unsigned)n_groups);
    if (P.S <= 128) sensor_grad_launch<128>(L, grid, s);
    else if (P.S <= 256) sensor_grad_launch<256>(L, grid, s);
    else if (P.S <= 384) sensor_grad_launch<384>(L, grid, s);
    else if (P.S <= 512) sensor_grad_launch<512>(L, grid, s);
    else sensor_grad_launch<640>(L, grid, s);
    sea_note_form("sensor_grad.rows64", 0, 0);
    sensor_sse_finish_kernel<<<dim3((unsigned)((P.Bm + 255) / 256)), dim3(256), 0, s>>>(P.work, P.wsse, P.Bm, (int)((int64_t)P.Q * n_groups));
    SEA_CHECK_LAUNCH("sea_decode_sensor_grad");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_derived_sensor_sse / sea_decode_derived_sensor_grad: sensors that read a DERIVED quantity — a speed, an energy, a difference of the two
// source values at one cell — scored (and differentiated) by the two kernels above compiled for the launch types with the pair tables.  A reading is
// two adjacent entries of the sorted, padded list: entry 2 i gathers the W2 row of source a, entry 2 i + 1 that of source b (same group, patch, cell).  A
// lane holds sorted positions 16 sub + 4 lg + r, r = 0 .. 3: two whole pairs, so the gathered tile load, both LDS images, the MFMA stage, the grid, the
// workspace and the finish launch are untouched and only the epilogue differs — in registers, no shuffles, no extra LDS (four tile images at SP = 640
// would need 168 kB).  op, scale, shift come per entry from device tables by 16-byte loads, as obs and prec do: a per-lane index into a by-value table
// in the kernel arguments would put that table into scratch.  x = dv_value(...) is the device function of the derived launches below; op == -1 at
// entry 2 i marks a plain reading (x = ya).  The weight, the observation and the residual of a pair are those of entry 2 i; pred gets x at both entries.
extern "C" int sea_decode_derived_sensor_sse(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeSensorSse* p, const SeaDerivedSensorTables* tables, int dtype,
                                             void* stream) {
    const char* who = "sea_decode_derived_sensor_sse";
    SEA_REQUIRE(p != nullptr, "%s: null argument table", who);
    const SeaDecodeSensorSse& P = *p;
    const int rc = sensor_args_check(who, groups, n_groups, P, nullptr, true, tables, dtype, "sea_gemm_grouped, a gather and the derived values in torch ops");
    if (rc != SEA_OK) return rc;

    DerivedSensorSseLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    L.t = *tables;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((int64_t)P.Bm + DM_ROWS - 1) / DM_ROWS), (unsigned)P.Q, (unsigned)n_groups);
    if (P.S <= 128) sensor_sse_launch<128>(L, grid, s);
    else if (P.S <= 256) sensor_sse_launch<256>(L, grid, s);
    else if (P.S <= 384) sensor_sse_launch<384>(L, grid, s);
    else if (P.S <= 512) sensor_sse_launch<512>(L, grid, s);
    else sensor_sse_launch<640>(L, grid, s);
    sea_note_form("derived_sensor_sse.rows64", 0, 0);
    sensor_sse_finish_kernel<<<dim3((unsigned)((P.Bm + 255) / 256)), dim3(256), 0, s>>>(P.work, P.wsse, P.Bm, (int)((int64_t)P.Q * n_groups));
    SEA_CHECK_LAUNCH(who);
    return SEA_OK;
}

extern "C" int sea_decode_derived_sensor_grad(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeSensorGrad* p, const SeaDerivedSensorTables* tables, int dtype,
                                              void* stream) {
    const char* who = "sea_decode_derived_sensor_grad";
    SEA_REQUIRE(p != nullptr, "%s: null argument table", who);
    const SeaDecodeSensorGrad& P = *p;
    const int rc = sensor_args_check(who, groups, n_groups, sensor_common(P), &P.grad_scale, true, tables, dtype,
                                     "sea_gemm_grouped, a gather and the derived values in torch ops under autograd");
    if (rc != SEA_OK) return rc;

    DerivedSensorGradLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    L.t = *tables;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(((int64_t)P.Bm + DM_ROWS - 1) / DM_ROWS), (unsigned)P.Q, (unsigned)n_groups);
    if (P.S <= 128) sensor_grad_launch<128>(L, grid, s);
    else if (P.S <= 256) sensor_grad_launch<256>(L, grid, s);
    else if (P.S <= 384) sensor_grad_launch<384>(L, grid, s);
    else if (P.S <= 512) sensor_grad_launch<512>(L, grid, s);
    else sensor_grad_launch<640>(L, grid, s);
    sea_note_form("derived_sensor_grad.rows64", 0, 0);
    sensor_sse_finish_kernel<<<dim3((unsigned)((P.Bm + 255) / 256)), dim3(256), 0, s>>>(P.work, P.wsse, P.Bm, (int)((int64_t)P.Q * n_groups));
    SEA_CHECK_LAUNCH(who);
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_field_grad: the DENSE-snapshot score with a per-cell precision map and per-field precisions, per member and field, WITH its gradient to the
// hidden rows — decode_mse_kernel (both MFMA stages over the same LDS image of W2, the [rows, 32 columns] tile of decoded values in accumulator registers
// between them) with the epilogue of the ensemble tools between the stages: the weight w = field_prec * prec applied by selects, the member -> observation
// row map of decode_member_sse_kernel, and per-row, per-field weighted sums in place of one scalar.  The workgroup (64 rows, 4 waves of 16), the H
// fragments, the SP masking, the two LDS images with the pitch of 2 SP + 32 bytes, both read forms, the prefetch of tile t + 1 around the MFMAs of tile t
// and the one barrier per tile are decode_mse_kernel's.  Per tile and wave:
//   before   the lane requests the observation AND the precision of its 2 x 4 columns (one float4 each per sub-tile, where the row has a valid column
//            there), and reads the field's precision (uniform),
//   stage 1  decode_mse_kernel's,
//   between  w = valid && pw > 0 && fw > 0 ? fw pw : 0;  d = w > 0 ? y - obs : 0  (selects: NaN, a negative value or Inf * 0 give no weight, and a cell
//            without weight is neutral whatever obs holds);  the lane's field sum += (w d) d in fp32;  r = bf16(w d), rounded ONCE: the A fragment of
//   stage 2  decode_mse_kernel's, into the wave's [16, SP] fp32 slice of dH.
// When the tile walk crosses a field boundary the lane's sum is folded over the four lanes that hold the row's columns (two butterfly steps, as
// decode_member_sse_kernel) and lane group 0 writes work[m, field0 + j]; member_sse_finish_kernel then adds the P rows of a member.  GRAD = false is the
// score-only form (no dH accumulators, no stage 2): the same stage 1 and the same epilogue arithmetic in the same order, so the score has the bits of
// the gradient launch.  One writer per dH and work element, no atomics: two runs give the same bits; a row of an MFMA result depends on its own operand
// row only, so a member's dH rows and wsse row do not depend on `members`, on the number of histories or on the 64-row tile the member falls into.
struct FieldGradLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeFieldGrad p;
};

template <int SP, bool GRAD>
__global__ __launch_bounds__(256) void decode_field_grad_kernel(const FieldGradLaunch L) {
#pragma clang fp reassociate(off)   // the lane's sum runs over its columns in the stated order, in both forms
    constexpr int KS = SP / 32;
    constexpr int ST = GRAD ? SP / 16 : 1;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = DM_TC * (SP / 8) / 256;
    static_assert(NCH * 256 == DM_TC * (SP / 8), "whole chunks per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images

    const SeaDecodeMseGroup& G = L.g[blockIdx.y];
    const SeaDecodeFieldGrad& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int M = P.M, S = P.S, C = P.C, Cp = P.Cp;
    const int row0 = blockIdx.x * DM_ROWS + wave * 16;
    const int m = row0 + li;   // the row this lane holds in the H fragments, in the stage-1 result and in the residual fragment
    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);

    // valid columns of this lane's row: [0, lim); its row of the observation: the `members` consecutive members of a history share one
    int lim = 0;
    int64_t tr = 0;
    if (m < M) {
        const int mem = m / P.P, patch = m - mem * P.P;
        lim = C;
        if (P.counts != nullptr) {
            const int cnt = P.counts[patch];
            lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
        }
        tr = (int64_t)(mem / P.members) * P.P + patch;
    }

    uint4 hf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int s = ks * 32 + 8 * lg;
        hf[ks] = make_uint4(0u, 0u, 0u, 0u);   // (not a ternary over two lvalues: that selects between ADDRESSES and puts the zero into scratch)
        if (m < M && s < S) hf[ks] = *reinterpret_cast<const uint4*>(H + (int64_t)m * G.ldh + s);
    }
    f32x4 dh[ST];
#pragma unroll
    for (int st = 0; st < ST; ++st) dh[st] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int tpf = (C + DM_TC - 1) / DM_TC;   // tiles of a field that hold real columns
    const int n_tiles = G.n_fields * tpf;
    uint4 wr[NCH];
    dm_load_tile<SP>(wr, W2, G.ldw, S, Cp, tpf, 0, tid);
    dm_store_tile<SP>(wr, smem, tid);
    __syncthreads();

    float fsum = 0.f;
    const float* orow = P.obs + tr * P.ld_row;
    const float* prow = P.prec != nullptr ? P.prec + tr * P.ld_row : nullptr;
    float* wrow = P.work + (int64_t)(m < M ? m : 0) * P.n_fields_total + G.field0;
    typedef dm_s16x4 __attribute__((address_space(3))) * lds_p;
    int j = 0, tj = 0;   // field of tile t and the tile's index inside it
    for (int t = 0; t < n_tiles; ++t) {
        const char* buf = smem + (t & 1) * TILE;
        if (t + 1 < n_tiles) dm_load_tile<SP>(wr, W2, G.ldw, S, Cp, tpf, t + 1, tid);
        const int cb = tj * DM_TC;

        // observation and precision of this lane's 2 x 4 columns (requested now, used after stage 1); a slot that is not read holds obs 0, precision 0
        float ob[2][4], pw[2][4];
        const int64_t foff = (int64_t)(G.field0 + j) * P.ld_field;
        const float fw = P.field_prec != nullptr ? P.field_prec[G.field0 + j] : 1.f;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const int c = cb + sub * 16 + 4 * lg;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                ob[sub][r] = 0.f;
                pw[sub][r] = 0.f;
            }
            if (c < lim) {
                if (c + 4 <= C) {
                    const float4 v = *reinterpret_cast<const float4*>(orow + foff + c);
                    ob[sub][0] = v.x; ob[sub][1] = v.y; ob[sub][2] = v.z; ob[sub][3] = v.w;
                    float4 q = make_float4(1.f, 1.f, 1.f, 1.f);
                    if (prow != nullptr) q = *reinterpret_cast<const float4*>(prow + foff + c);
                    pw[sub][0] = q.x; pw[sub][1] = q.y; pw[sub][2] = q.z; pw[sub][3] = q.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (c + r < C) {
                            ob[sub][r] = orow[foff + c + r];
                            pw[sub][r] = prow != nullptr ? prow[foff + c + r] : 1.f;
                        }
                }
            }
        }

        // stage 1
        f32x4 acc[2][2];
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
            const float4 b = *reinterpret_cast<const float4*>(G.bias + j * Cp + cb + sub * 16 + 4 * lg);
            acc[sub][0] = f32x4{b.x, b.y, b.z, b.w};
            acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            if (ks * 32 < S) {
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    const uint4 a = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                    mma16<__bf16>(a, hf[ks], acc[sub][ks & 1]);
                }
            }
        }

        // weight and residual by selects, the field's weighted square sum, the weighted residual rounded once
        bf16x8 dfr;
#pragma unroll
        for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = cb + sub * 16 + 4 * lg + r;
                const float p = pw[sub][r];
                const float w = (c < lim && p > 0.f && fw > 0.f) ? mul1(fw, p) : 0.f;
                const float y = acc[sub][0][r] + acc[sub][1][r];
                const float d = w > 0.f ? y - ob[sub][r] : 0.f;
                const float wd = mul1(w, d);
                fsum = fma1(wd, d, fsum);
                dfr[sub * 4 + r] = (__bf16)wd;
            }
        }

        if (GRAD) {   // stage 2
            const uint4 da = __builtin_bit_cast(uint4, dfr);
            const char* tb = buf + (4 * lg + (li >> 2)) * PITCH + (4 * (li & 3)) * 2;
#pragma unroll
            for (int st = 0; st < ST; ++st) {
                if (st * 16 < S) {
                    const dm_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(tb + st * 32));
                    const dm_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(tb + st * 32 + 16 * PITCH));
                    const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                    mma16<__bf16>(da, make_uint4(l2.x, l2.y, h2.x, h2.y), dh[st]);
                }
            }
        }

        if (++tj == tpf) {   // the field is complete (uniform over the workgroup): fold the row's four lanes, one writer
            float v = fsum;
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            if (lg == 0 && m < M) wrow[j] = v;
            fsum = 0.f;
            tj = 0;
            ++j;
        }

        if (t + 1 < n_tiles) dm_store_tile<SP>(wr, smem + ((t + 1) & 1) * TILE, tid);
        __syncthreads();
    }

    if (GRAD) {   // dH: register r of tile st is row 4 g + r of the wave, column 16 st + (lane & 15)
        const float scale = 2.0f * P.grad_scale;
        __bf16* dH = static_cast<__bf16*>(G.dH);
        const __bf16* Z = static_cast<const __bf16*>(G.Z);
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const int s = st * 16 + li;
            if (s < S) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int mr = row0 + 4 * lg + r;
                    if (mr < M) {
                        float v = dh[st][r] * scale;
                        if (Z != nullptr) v *= gelu_grad_for<__bf16>((float)Z[(int64_t)mr * G.ldz + s]);
                        dH[(int64_t)mr * G.lddh + s] = (__bf16)v;
                    }
                }
            }
        }
    }
}

template <int SP, bool GRAD>
static void field_grad_launch(const FieldGradLaunch& L, dim3 grid, hipStream_t s) {
    constexpr int lds = 2 * DM_TC * (SP * 2 + DM_PAD);
    static bool set_on[64] = {false};   // per device: SP = 640 needs 84 kB, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_field_grad_kernel<SP, GRAD>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_field_grad_kernel<SP, GRAD><<<grid, dim3(256), lds, s>>>(L);
}

template <bool GRAD>
static void field_grad_dispatch(const FieldGradLaunch& L, dim3 grid, hipStream_t s) {
    const int S = L.p.S;
    if (S <= 128) field_grad_launch<128, GRAD>(L, grid, s);
    else if (S <= 256) field_grad_launch<256, GRAD>(L, grid, s);
    else if (S <= 384) field_grad_launch<384, GRAD>(L, grid, s);
    else if (S <= 512) field_grad_launch<512, GRAD>(L, grid, s);
    else field_grad_launch<640, GRAD>(L, grid, s);
}

extern "C" int sea_decode_field_grad(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeFieldGrad* p, int dtype, void* stream) {
    SEA_REQUIRE(groups != nullptr && p != nullptr, "sea_decode_field_grad: null argument table");
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "sea_decode_field_grad: n_groups=%d outside 1..%d", n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "sea_decode_field_grad: bad dtype %d", dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("sea_decode_field_grad: unsupported: bf16 only (the fp32 decoder composes sea_gemm_grouped and reductions under autograd)");
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeFieldGrad& P = *p;
    SEA_REQUIRE(P.obs != nullptr && P.wsse != nullptr && P.work != nullptr, "sea_decode_field_grad: null obs, wsse or work pointer");
    SEA_REQUIRE(P.M >= 1, "sea_decode_field_grad: M=%d must be positive", P.M);
    SEA_REQUIRE(P.S >= 8 && P.S % 8 == 0, "sea_decode_field_grad: S=%d must be a positive multiple of 8", P.S);
    SEA_REQUIRE(P.Cp >= 32 && P.Cp % 32 == 0, "sea_decode_field_grad: Cp=%d must be a positive multiple of 32", P.Cp);
    SEA_REQUIRE(P.C >= 1 && P.C <= P.Cp, "sea_decode_field_grad: C=%d must lie in 1..Cp=%d", P.C, P.Cp);
    SEA_REQUIRE(P.P >= 1 && P.members >= 1, "sea_decode_field_grad: P=%d and members=%d must be positive", P.P, P.members);
    SEA_REQUIRE((int64_t)P.M % ((int64_t)P.P * P.members) == 0, "sea_decode_field_grad: M=%d is not a multiple of P * members = %d * %d", P.M, P.P, P.members);
    SEA_REQUIRE(P.n_fields_total >= 1, "sea_decode_field_grad: n_fields_total=%d must be positive", P.n_fields_total);
    SEA_REQUIRE(P.work_cap >= (int64_t)P.M * P.n_fields_total, "sea_decode_field_grad: workspace of %lld floats is too small: %lld needed (M * n_fields_total)",
                (long long)P.work_cap, (long long)((int64_t)P.M * P.n_fields_total));
    SEA_REQUIRE(P.ld_row >= 0 && P.ld_row % 4 == 0 && P.ld_field >= 0 && P.ld_field % 4 == 0,
                "sea_decode_field_grad: obs strides ld_row=%lld, ld_field=%lld must be multiples of 4", (long long)P.ld_row, (long long)P.ld_field);
    SEA_REQUIRE(sea_aligned16(P.obs) && sea_aligned16(P.prec), "sea_decode_field_grad: obs and prec must be 16-byte aligned");
    SEA_REQUIRE(sea_aligned4(P.field_prec) && sea_aligned4(P.counts) && sea_aligned4(P.wsse) && sea_aligned4(P.work),
                "sea_decode_field_grad: misaligned field_prec, counts, wsse or work pointer");
    uint32_t gs_bits;
    memcpy(&gs_bits, &P.grad_scale, sizeof(gs_bits));
    SEA_REQUIRE((gs_bits & 0x7f800000u) != 0x7f800000u, "sea_decode_field_grad: grad_scale must be finite");   // the exponent field itself: no floating-point compare to reason about
    int64_t covered = 0;
    int with_dh = 0;
    for (int g = 0; g < n_groups; ++g) with_dh += groups[g].dH != nullptr ? 1 : 0;
    for (int g = 0; g < n_groups; ++g) {
        const SeaDecodeMseGroup& G = groups[g];
        SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr, "sea_decode_field_grad: group %d: null pointer (H, W2 or bias)", g);
        SEA_REQUIRE(with_dh == 0 || G.dH != nullptr, "sea_decode_field_grad: group %d: dH is NULL but %d other groups carry one (all groups, or none for the score alone)", g, with_dh);
        SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias) && sea_aligned16(G.dH), "sea_decode_field_grad: group %d: pointers must be 16-byte aligned", g);
        SEA_REQUIRE(G.ldh >= P.S && G.ldh % 8 == 0 && G.ldw >= P.S && G.ldw % 8 == 0,
                    "sea_decode_field_grad: group %d: row strides ldh=%d ldw=%d must cover S=%d and be multiples of 8", g, G.ldh, G.ldw, P.S);
        if (with_dh != 0) {
            SEA_REQUIRE(sea_aligned16(G.Z), "sea_decode_field_grad: group %d: Z must be 16-byte aligned", g);
            SEA_REQUIRE(G.lddh >= P.S && G.lddh % 2 == 0 && (G.Z == nullptr || G.ldz >= P.S),
                        "sea_decode_field_grad: group %d: row strides lddh=%d ldz=%d must cover S=%d (lddh even)", g, G.lddh, G.ldz, P.S);
        }
        SEA_REQUIRE(G.n_fields >= 1 && G.field0 >= 0 && (int64_t)G.field0 + G.n_fields <= P.n_fields_total,
                    "sea_decode_field_grad: group %d: n_fields=%d, field0=%d outside the %d fields", g, G.n_fields, G.field0, P.n_fields_total);
        SEA_REQUIRE((int64_t)G.n_fields * P.Cp <= 0x7fffffffLL / 2, "sea_decode_field_grad: group %d: too many output columns", g);
        for (int h = 0; h < g; ++h)
            SEA_REQUIRE(G.field0 >= groups[h].field0 + groups[h].n_fields || groups[h].field0 >= G.field0 + G.n_fields,
                        "sea_decode_field_grad: group %d: its fields overlap those of group %d (every output element has one writer)", g, h);
        covered += G.n_fields;
    }
    SEA_REQUIRE(covered == P.n_fields_total, "sea_decode_field_grad: the groups cover %lld of the %d fields (every field needs exactly one group)", (long long)covered, P.n_fields_total);
    if (P.S > 640) {
        sea_set_error("sea_decode_field_grad: unsupported: hidden width S=%d above 640", P.S);
        return SEA_EUNSUPPORTED;
    }
    const int64_t row_blocks = ((int64_t)P.M + DM_ROWS - 1) / DM_ROWS;
    const int64_t n_out = (int64_t)(P.M / P.P) * P.n_fields_total;
    SEA_REQUIRE(row_blocks <= 0x7fffffffLL && (n_out + 3) / 4 <= 0x7fffffffLL, "sea_decode_field_grad: too many rows");

    FieldGradLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)row_blocks, (unsigned)n_groups);
    if (with_dh != 0) field_grad_dispatch<true>(L, grid, s);
    else field_grad_dispatch<false>(L, grid, s);
    sea_note_form("field_grad.rows64", with_dh != 0 ? 1 : 0, 0);
    member_sse_finish_kernel<<<dim3((unsigned)((n_out + 3) / 4)), dim3(256), 0, s>>>(P.work, P.wsse, n_out, P.P, P.n_fields_total);
    SEA_CHECK_LAUNCH("sea_decode_field_grad");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_member_gram: what the ensemble Kalman analysis needs from a DENSE observation of the decoded fields — per (history, patch) the N x N Gram
// matrix of the members' weighted decoded anomalies and its product with the innovation (include/sea_hip.h states the formulas).  The walk is
// decode_member_moments_kernel's: one workgroup of 8 waves serves one (history, patch), wave w decodes the members 16 w .. 16 w + 15 tile by tile (32
// columns of one field; stage 1 of decode_mse_kernel, the bias in the accumulator), and the decoded values never leave the chip.  The field groups are
// looped INSIDE the workgroup in ascending order, so one launch finishes gram, proj and count.  Per tile:
//   a  the wave's column sums over its live members (four per lane, two butterfly steps over the lane groups) go to LDS; after a barrier every lane adds
//      the 8 waves' sums of its column in ascending order and scales by 1 / N: ybar, the same bits in every wave.  A member row at or beyond N is passed
//      over by a select (its hidden row is zero, so its decoded "value" is the bias: it must not reach the mean, and its anomaly must be 0, not -ybar);
//   b  the weight of the column w = valid ? max(pf, 0) max(prec, 0) : 0 by selects (a NaN compares false); the lane forms x_j = sqrt(w) (y_j - ybar) and
//      e = sqrt(w) (obs - ybar) in fp32 — both exactly 0 where w is not positive, whatever obs, prec or the pad columns hold — adds x_j e to its four fp64
//      proj sums, and writes x_j to an LDS image X[member][32 columns];
//   c  G += X X^T over the tile's 32 columns with the f32-input MFMA (v_mfma_f32_16x16x4_f32: bit for bit an ordered fmaf chain, so the fp32 sum stays
//      inside ONE tile, in two chains of four k-steps), each 16 x 16 block then added to fp64 accumulators in registers — everything across tiles,
//      fields and groups is fp64, in ascending (group, field, tile) order.  Both operands of a block are rows of the same image and sqrt(w) sits on
//      both sides, so the product commutes: block (i, j) and block (j, i) have the same bits, and only the blocks of a circulant half are computed:
//      wave w owns (w, (w + d) mod NB) for d = 0 .. NB / 2 (at d = NB / 2 with NB even only the waves below d), 4 or 5 blocks at 128 members; the
//      mirror block is stored from the same registers, the diagonal blocks are symmetric by the commuting fmaf chain.
// count: wave 0 counts the columns with w > 0.  A live column whose obs or whose live member value is not finite, or a stored sum that is not finite,
// sets count = -1.  No atomics, one writer per element (an off-diagonal block and its mirror have the one owner): two runs give the same bits, and
// nothing of a (history, patch) depends on the others.  A patch without a valid column writes zeros and leaves before any barrier.
struct MemberGramLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeMemberGram p;
    int n_groups;
    float inv_n;
};

constexpr int MG_NW = 8;        // waves per workgroup: 128 members
constexpr int MG_XP = 36;       // floats per row of the anomaly image (32 columns + 4: 16-byte rows)
constexpr int MG_MAXD = 5;      // circulant offsets a wave may own: d = 0 .. 4 at 8 blocks

template <int SP>
constexpr int mg_lds_bytes() { return 2 * DM_TC * (SP * 2 + DM_PAD) + MG_NW * DM_TC * 4 + 16 * MG_NW * MG_XP * 4; }

template <int SP>
__global__ __launch_bounds__(64 * MG_NW) void decode_member_gram_kernel(const MemberGramLaunch L) {
#pragma clang fp reassociate(off)
    constexpr int NW = MG_NW;
    constexpr int NT = 64 * NW;
    constexpr int KS = SP / 32;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    constexpr int XP = MG_XP;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    static_assert(16 * NW * XP * 4 >= NW * 16 * 16 * 8, "the proj fold fits the anomaly image");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images; the waves' column sums [NW][32]; the anomaly image [128][XP]
    float* red = reinterpret_cast<float*>(smem + 2 * TILE);
    float* Xs = reinterpret_cast<float*>(smem + 2 * TILE + NW * DM_TC * 4);

    const SeaDecodeMemberGram& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
    const int S = P.S, C = P.C, Cp = P.Cp, N = P.members;
    const int bp = blockIdx.x;
    const int b = bp / P.P, patch = bp - b * P.P;
    double* const o_gram = P.gram + (int64_t)bp * N * N;
    double* const o_proj = P.proj + (int64_t)bp * N;

    int lim = C;   // valid columns of this patch: [0, lim) — uniform over the workgroup
    if (P.counts != nullptr) {
        const int cnt = P.counts[patch];
        lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
    }
    const int tpf = (lim + DM_TC - 1) / DM_TC;   // tiles of a field that hold valid columns
    if (tpf == 0) {   // uniform: before any barrier
        for (int i = tid; i < N * N; i += NT) o_gram[i] = 0.0;
        if (tid < N) o_proj[tid] = 0.0;
        if (tid == 0) P.count[bp] = 0;
        return;
    }

    const int NB = (N + 15) >> 4;               // 16-member blocks
    const int j0 = wave * 16;
    const bool active = j0 < N;                 // uniform over the wave
    const int nrow = N - (j0 + 4 * lg);         // the lane's accumulator rows r < nrow are members
    const int jm = j0 + li;
    const bool row_live = jm < N;
    const int64_t m = ((int64_t)b * N + (row_live ? jm : 0)) * P.P + patch;

    double gacc[MG_MAXD][4], pacc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        pacc[r] = 0.0;
#pragma unroll
        for (int d = 0; d < MG_MAXD; ++d) gacc[d][r] = 0.0;
    }
    int bad = 0, ncell = 0;

    for (int gi = 0; gi < L.n_groups; ++gi) {
        const SeaDecodeMseGroup& G = L.g[gi];
        const __bf16* H = static_cast<const __bf16*>(G.H);
        const __bf16* W2 = static_cast<const __bf16*>(G.W2);
        uint4 hf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int s = ks * 32 + 8 * lg;
            // a row at or beyond N repeats member 0's: whatever it decodes to is passed over by the selects of b.  Whole k-steps below S load plainly (a
            // uniform branch); the step that straddles S loads column 0 where s >= S and selects zeros (the tile image is zero there, but 0 * NaN is not)
            if (ks * 32 + 32 <= S) {
                hf[ks] = *reinterpret_cast<const uint4*>(H + m * G.ldh + s);
            } else {
                const uint4 v = *reinterpret_cast<const uint4*>(H + m * G.ldh + (s < S ? s : 0));
                hf[ks] = s < S ? v : make_uint4(0u, 0u, 0u, 0u);
            }
        }
        const int n_tiles = G.n_fields * tpf;
        uint4 wr[NCH];
        dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, 0, tid);
        dm_store_tile<SP, NT>(wr, smem, tid);   // the group before this one ended on a barrier: image 0 is free
        __syncthreads();

        int j = 0, tj = 0;   // field of tile t inside the group and the tile's index inside the field
        for (int t = 0; t < n_tiles; ++t) {
            const char* buf = smem + (t & 1) * TILE;
            const int cb = tj * DM_TC;
            const int fg = G.field0 + j;

            // a: decode, the wave's column sums
            float y[2][4];
            if (active) {
                f32x4 acc[2][2];
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    const float bv = G.bias[j * Cp + cb + sub * 16 + li];
                    acc[sub][0] = f32x4{bv, bv, bv, bv};
                    acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    if (ks * 32 < S) {
#pragma unroll
                        for (int sub = 0; sub < 2; ++sub) {
                            const uint4 wv = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                            mma16<__bf16>(hf[ks], wv, acc[sub][ks & 1]);
                        }
                    }
                }
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    float sm = 0.f;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        y[sub][r] = acc[sub][0][r] + acc[sub][1][r];   // plain C++: the first reader of an MFMA result must be an instruction the compiler sees
                        sm = (r < nrow) ? add1(sm, y[sub][r]) : sm;
                    }
                    sm = add1(sm, __shfl_xor(sm, 16));
                    sm = add1(sm, __shfl_xor(sm, 32));
                    if (lg == 0) red[wave * DM_TC + sub * 16 + li] = sm;
                }
            } else {
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[sub][r] = 0.f;
                }
                if (lane < DM_TC) red[wave * DM_TC + lane] = 0.f;
            }
            __syncthreads();
            if (t + 1 < n_tiles) dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t + 1, tid);   // in flight behind b and c; not alive beside a's accumulators

            // b: the mean, the weights, the anomalies
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const int cl = sub * 16 + li, c = cb + cl;
                float ys = red[cl];
#pragma unroll
                for (int w = 1; w < NW; ++w) ys = add1(ys, red[w * DM_TC + cl]);
                const float ybar = mul1(ys, L.inv_n);
                float w = 0.f;
                if (c < lim) {
                    const float pf = P.prec_field != nullptr ? P.prec_field[fg] : 1.f;
                    const float pm = P.prec != nullptr ? P.prec[(int64_t)bp * P.ld_prow + (int64_t)fg * P.ld_pfield + c] : 1.f;
                    w = mul1(pf > 0.f ? pf : 0.f, pm > 0.f ? pm : 0.f);
                }
                const bool on = w > 0.f;   // false for NaN
                const float ov = on ? P.obs[(int64_t)bp * P.ld_row + (int64_t)fg * P.ld_field + c] : 0.f;
                const float sw = on ? sqrtf(w) : 0.f;
                const float e = on ? mul1(sw, add1(ov, -ybar)) : 0.f;
                if (on && !isfinite(e)) bad = 1;
                if (on && wave == 0 && lg == 0) ++ncell;
                if (active) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float x = (on && (r < nrow)) ? mul1(sw, add1(y[sub][r], -ybar)) : 0.f;
                        if (on && (r < nrow) && !isfinite(x)) bad = 1;
                        pacc[r] = fma((double)x, (double)e, pacc[r]);
                        Xs[(j0 + 4 * lg + r) * XP + cl] = x;
                    }
                }
            }
            __syncthreads();

            // c: the blocks of X X^T this wave owns
            if (wave < NB) {
                const float4 a0 = *reinterpret_cast<const float4*>(Xs + (j0 + li) * XP + 8 * lg);
                const float4 a1 = *reinterpret_cast<const float4*>(Xs + (j0 + li) * XP + 8 * lg + 4);
#pragma unroll
                for (int d = 0; d < MG_MAXD; ++d) {
                    if (2 * d <= NB && (2 * d != NB || wave < d)) {   // uniform over the wave
                        int bj = wave + d;
                        bj = bj >= NB ? bj - NB : bj;
                        const float4 b0 = *reinterpret_cast<const float4*>(Xs + (bj * 16 + li) * XP + 8 * lg);
                        const float4 b1 = *reinterpret_cast<const float4*>(Xs + (bj * 16 + li) * XP + 8 * lg + 4);
                        f32x4 c0 = f32x4{0.f, 0.f, 0.f, 0.f}, c1 = f32x4{0.f, 0.f, 0.f, 0.f};
                        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b0.x, c0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b1.x, c1, 0, 0, 0);
                        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b0.y, c0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b1.y, c1, 0, 0, 0);
                        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b0.z, c0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b1.z, c1, 0, 0, 0);
                        c0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b0.w, c0, 0, 0, 0);
                        c1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b1.w, c1, 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < 4; ++r) gacc[d][r] += (double)c0[r] + (double)c1[r];
                    }
                    if constexpr (SP > 512) __builtin_amdgcn_sched_barrier(0);   // one block's fragments at a time: with all five hoisted the widest form spills
                }
            }
            if (++tj == tpf) {
                tj = 0;
                ++j;
            }
            if (t + 1 < n_tiles) dm_store_tile<SP, NT>(wr, smem + ((t + 1) & 1) * TILE, tid);
            __syncthreads();
        }
    }

    // the blocks and their mirrors: row 16 wave + 4 lg + r, column 16 bj + li
    if (wave < NB) {
#pragma unroll
        for (int d = 0; d < MG_MAXD; ++d) {
            if (2 * d <= NB && (2 * d != NB || wave < d)) {
                int bj = wave + d;
                bj = bj >= NB ? bj - NB : bj;
                const int col = bj * 16 + li;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = j0 + 4 * lg + r;
                    if (row < N && col < N) {
                        const double v = gacc[d][r];
                        if (!isfinite(v)) bad = 1;
                        o_gram[(int64_t)row * N + col] = v;
                        if (d != 0) o_gram[(int64_t)col * N + row] = v;
                    }
                }
            }
        }
    }
    // proj: the 16 column lanes of a member in ascending order, through the anomaly image's memory (the loop above ended on a barrier)
    double* ps = reinterpret_cast<double*>(Xs);
#pragma unroll
    for (int r = 0; r < 4; ++r) ps[(j0 + 4 * lg + r) * 16 + li] = pacc[r];
    int* cs = reinterpret_cast<int*>(red);
    if (wave == 0 && lg == 0) cs[li] = ncell;
    __syncthreads();
    if (tid < N) {
        double s = 0.0;
        for (int i = 0; i < 16; ++i) s += ps[tid * 16 + i];
        if (!isfinite(s)) bad = 1;
        o_proj[tid] = s;
    }
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        int n = 0;
        for (int i = 0; i < 16; ++i) n += cs[i];
        P.count[bp] = bad ? -1 : n;
    }
}

template <int SP>
static void member_gram_launch(const MemberGramLaunch& L, dim3 grid, hipStream_t s) {
    constexpr int lds = mg_lds_bytes<SP>();
    static bool set_on[64] = {false};   // per device: SP = 640 needs 103 kB, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_member_gram_kernel<SP>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_member_gram_kernel<SP><<<grid, dim3(64 * MG_NW), lds, s>>>(L);
    sea_note_form("decode.member_gram", SP, lds);
}

extern "C" int sea_decode_member_gram(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberGram* p, int dtype, void* stream) {
    SEA_REQUIRE(groups != nullptr && p != nullptr, "sea_decode_member_gram: null argument table");
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "sea_decode_member_gram: n_groups=%d outside 1..%d", n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "sea_decode_member_gram: bad dtype %d", dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("sea_decode_member_gram: unsupported: bf16 only (the fp32 decoder composes sea_gemm_grouped and fp64 reductions)");
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeMemberGram& P = *p;
    SEA_REQUIRE(P.obs != nullptr && P.gram != nullptr && P.proj != nullptr && P.count != nullptr,
                "sea_decode_member_gram: null pointer (obs, gram, proj and count are required; prec_field, prec and counts may be NULL)");
    SEA_REQUIRE(P.M >= 1, "sea_decode_member_gram: M=%d must be positive", P.M);
    SEA_REQUIRE(P.S >= 8 && P.S % 8 == 0, "sea_decode_member_gram: S=%d must be a positive multiple of 8", P.S);
    SEA_REQUIRE(P.Cp >= 32 && P.Cp % 32 == 0, "sea_decode_member_gram: Cp=%d must be a positive multiple of 32", P.Cp);
    SEA_REQUIRE(P.C >= 1 && P.C <= P.Cp, "sea_decode_member_gram: C=%d must lie in 1..Cp=%d", P.C, P.Cp);
    SEA_REQUIRE(P.P >= 1, "sea_decode_member_gram: P=%d must be positive", P.P);
    SEA_REQUIRE(P.members >= 2, "sea_decode_member_gram: members=%d: an analysis needs at least 2 members", P.members);
    SEA_REQUIRE((int64_t)P.M % ((int64_t)P.P * P.members) == 0, "sea_decode_member_gram: M=%d is not a multiple of P * members = %d * %d", P.M, P.P, P.members);
    SEA_REQUIRE(P.n_fields_total >= 1, "sea_decode_member_gram: n_fields_total=%d must be positive", P.n_fields_total);
    SEA_REQUIRE(P.ld_field >= P.C && P.ld_row >= 0, "sea_decode_member_gram: obs strides ld_row=%lld, ld_field=%lld must cover C=%d", (long long)P.ld_row,
                (long long)P.ld_field, P.C);
    SEA_REQUIRE(P.prec == nullptr || (P.ld_pfield >= P.C && P.ld_prow >= 0), "sea_decode_member_gram: prec strides ld_prow=%lld, ld_pfield=%lld must cover C=%d",
                (long long)P.ld_prow, (long long)P.ld_pfield, P.C);
    SEA_REQUIRE(sea_aligned4(P.obs) && sea_aligned4(P.prec_field) && sea_aligned4(P.prec) && sea_aligned4(P.counts) && sea_aligned4(P.count) &&
                    (reinterpret_cast<uintptr_t>(P.gram) & 7u) == 0 && (reinterpret_cast<uintptr_t>(P.proj) & 7u) == 0,
                "sea_decode_member_gram: misaligned obs, prec_field, prec, counts, count (4 bytes), gram or proj (8 bytes) pointer");
    int64_t covered = 0;
    for (int g = 0; g < n_groups; ++g) {
        const SeaDecodeMseGroup& G = groups[g];
        SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr, "sea_decode_member_gram: group %d: null pointer", g);
        SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias), "sea_decode_member_gram: group %d: pointers must be 16-byte aligned", g);
        SEA_REQUIRE(G.ldh >= P.S && G.ldh % 8 == 0 && G.ldw >= P.S && G.ldw % 8 == 0,
                    "sea_decode_member_gram: group %d: row strides ldh=%d ldw=%d must cover S=%d and be multiples of 8", g, G.ldh, G.ldw, P.S);
        SEA_REQUIRE(G.n_fields >= 1 && G.field0 >= 0 && (int64_t)G.field0 + G.n_fields <= P.n_fields_total,
                    "sea_decode_member_gram: group %d: n_fields=%d, field0=%d outside the %d fields", g, G.n_fields, G.field0, P.n_fields_total);
        SEA_REQUIRE((int64_t)G.n_fields * P.Cp <= 0x7fffffffLL / 2, "sea_decode_member_gram: group %d: too many output columns", g);
        for (int h = 0; h < g; ++h)
            SEA_REQUIRE(G.field0 >= groups[h].field0 + groups[h].n_fields || groups[h].field0 >= G.field0 + G.n_fields,
                        "sea_decode_member_gram: group %d: its fields overlap those of group %d (a cell is counted once)", g, h);
        covered += G.n_fields;
    }
    SEA_REQUIRE(covered == P.n_fields_total, "sea_decode_member_gram: the groups cover %lld of the %d fields (every field needs exactly one group)", (long long)covered, P.n_fields_total);
    if (P.S > 640) {
        sea_set_error("sea_decode_member_gram: unsupported: hidden width S=%d above 640", P.S);
        return SEA_EUNSUPPORTED;
    }
    if (P.members > 16 * MG_NW) {
        sea_set_error("sea_decode_member_gram: unsupported: members=%d above %d", P.members, 16 * MG_NW);
        return SEA_EUNSUPPORTED;
    }
    const int64_t BP = (int64_t)P.M / P.members;   // (history, patch) pairs
    SEA_REQUIRE(BP <= 0x7fffffffLL, "sea_decode_member_gram: too many rows");

    MemberGramLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    L.n_groups = n_groups;
    L.inv_n = 1.0f / (float)P.members;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)BP);
    if (P.S <= 128) member_gram_launch<128>(L, grid, s);
    else if (P.S <= 256) member_gram_launch<256>(L, grid, s);
    else if (P.S <= 384) member_gram_launch<384>(L, grid, s);
    else if (P.S <= 512) member_gram_launch<512>(L, grid, s);
    else member_gram_launch<640>(L, grid, s);
    SEA_CHECK_LAUNCH("sea_decode_member_gram");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_member_verify: verification of an ensemble against a DENSE observation of the decoded fields — per cell the ensemble mean, spread, CRPS,
// PIT and rank, per (history, field) the fp64 sums and the rank histogram (include/sea_hip.h states the formulas; they are sea_ensemble_verify's with a
// cell for a sensor).  Launch 1 has decode_member_gram_kernel's walk, with one workgroup of 8 waves per (history, patch, FIELD, chunk of MV_CHUNK
// tiles of the field) — grid.y is the field, grid.z the chunk: the sums are per field anyway, scoring and not decoding sets the time, and at one
// history a workgroup per (history, patch) would leave three quarters of the chip idle behind a chain of n_fields * tiles scoring steps whose length
// the fullest patch sets.  A chunk without a valid column leaves at once.  Wave w decodes the members 16 w .. 16 w + 15 tile by tile (32 columns
// of the field).  Per tile:
//   a  threads 0 .. 31 form the columns' weights (decode_member_gram_kernel's selects) and read obs where the weight is positive; the waves decode and
//      write their values to an LDS image V[column][member] with a row of 129 floats (an odd stride: the lane-per-member reads of b are conflict-free
//      and the walk's reads are broadcasts; the stores of a, four rows apart per lane group, pay a two-way conflict once per tile);
//   b  wave w scores the columns w, w + 8, w + 16, w + 24 with vf_score_wave (verify_score.hpp: the arithmetic verify_kernel runs per sensor, in fp64,
//      members compared as the f32 values they are); a dead column is passed over by its wave;
//   c  thread k finishes column k (vf_finish_reading), stores the five maps — one writer per element, 128-byte segments — files the column's eight
//      terms and counts its rank in the field's LDS histogram (integer adds); the next tile of W2 goes to its LDS image meanwhile;
//   d  threads 0 .. 7 add the tile's terms in ascending column order onto the field's running fp64 sums; after the last tile the sums and the
//      histogram go to `work` [(history, patch), chunk, field].
// Three barriers per tile.  Columns at or beyond the walked tiles (whole tiles of invalid or pad columns) are filled as dead before the walk.
// member_verify_finish_kernel: one workgroup per history adds the partials of each field in ascending (patch, chunk) order.
// No floating-point atomics anywhere, no exchange between workgroups: two runs give the same bits, a history's outputs are those of a call holding it
// alone, and a cell's own outputs depend on its column of V, its weight and its reading only.
struct MemberVerifyLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeMemberVerify p;
    int n_groups;
    int words;   // 8-byte words per (history, patch, field) of the workspace
};

constexpr int MV_NW = 8;               // waves per workgroup: 128 members
constexpr int MV_NT = 64 * MV_NW;
constexpr int MV_VP = VF_MAX_N + 1;    // floats per column of the value image
constexpr int MV_CHUNK = 16;           // tiles (of 32 columns) of a field that one workgroup scores

static inline int mv_chunks(int Cp) { return (Cp / DM_TC + MV_CHUNK - 1) / MV_CHUNK; }

static inline int64_t mv_words(int N) { return VF_SUMS + (N + 2) / 2; }   // 8 sums, then N + 1 int32 bins

// LDS at SP = 640: 2 x 41984 (W2 images) + 16512 (V) dynamic, 6.6 kB static (weights, readings, terms, histogram): 107 kB of the CU's 160 kB
template <int SP>
constexpr int mv_lds_bytes() { return 2 * DM_TC * (SP * 2 + DM_PAD) + DM_TC * MV_VP * 4; }

template <int SP, int V>
__global__ __launch_bounds__(MV_NT) void decode_member_verify_kernel(const MemberVerifyLaunch L) {
#pragma clang fp reassociate(off)
    constexpr int NW = MV_NW;
    constexpr int NT = MV_NT;
    constexpr int KS = SP / 32;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    constexpr int VP = MV_VP;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images; the value image [32][VP]
    float* Vs = reinterpret_cast<float*>(smem + 2 * TILE);
    __shared__ double lw_s[VF_MAX_N], w_s[VF_MAX_N];
    __shared__ int live_s[VF_MAX_N];
    __shared__ VfReading r_s[DM_TC];
    __shared__ double term_s[VF_SUMS][DM_TC];
    __shared__ int hist_s[VF_MAX_N + 1];
    __shared__ float y_s[DM_TC], pv_s[DM_TC];

    const SeaDecodeMemberVerify& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
    const int S = P.S, C = P.C, Cp = P.Cp, N = P.members, F = P.n_fields_total, words = L.words;
    const int bp = blockIdx.x, fg = blockIdx.y, ck = blockIdx.z, Q = gridDim.z;   // the field and the chunk of its tiles this workgroup scores
    const int b = bp / P.P, patch = bp - b * P.P;
    const int64_t ld = P.ld_out;
    const int64_t obase = ((int64_t)bp * F + fg) * ld;
    double* const wsum = reinterpret_cast<double*>(P.work) + (((int64_t)bp * Q + ck) * F + fg) * words;
    int32_t* const whist = reinterpret_cast<int32_t*>(wsum + VF_SUMS);

    int lim = C;   // valid columns of this patch: [0, lim) — uniform over the workgroup
    if (P.counts != nullptr) {
        const int cnt = P.counts[patch];
        lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
    }
    const int tpf = (lim + DM_TC - 1) / DM_TC;   // tiles of a field that hold valid columns
    const int tb = ck * MV_CHUNK, te = tpf < tb + MV_CHUNK ? tpf : tb + MV_CHUNK;   // this workgroup's tiles: [tb, te)

    // the weights of the history (verify_kernel's step 1)
    int invalid = 0, alive = 0;
    if (tid < N) {
        const float lw = P.logw != nullptr ? P.logw[(int64_t)b * N + tid] : 0.f;
        invalid = (lw != lw || lw == INFINITY) ? 1 : 0;
        alive = (!invalid && lw != -INFINITY) ? 1 : 0;
        lw_s[tid] = (double)lw;
        live_s[tid] = alive;
    }
    for (int r = tid; r <= N; r += NT) hist_s[r] = 0;
    const int n_live = __syncthreads_count(alive);
    invalid = __syncthreads_or(invalid);
    const bool unscored = invalid || n_live == 0;
    if (patch == 0 && fg == 0 && ck == 0 && tid == 0) P.status[b] = unscored ? -1 : n_live;
    if (ck == 0) {   // the columns no tile walks (all of them when the history is not scored or the patch has no valid column): dead
        const int c0 = (unscored || tpf == 0) ? 0 : tpf * DM_TC;
        for (int64_t c = c0 + tid; c < ld; c += NT) {
            const int64_t at = obase + c;
            if (P.mean != nullptr) P.mean[at] = 0.f;
            if (P.spread != nullptr) P.spread[at] = 0.f;
            if (P.crps != nullptr) P.crps[at] = 0.f;
            if (P.pit != nullptr) P.pit[at] = 0.f;
            if (P.rank != nullptr) P.rank[at] = -1;
        }
    }
    if (unscored || te <= tb) {   // uniform: nothing to score in this chunk
        for (int e = tid; e < words; e += NT) wsum[e] = 0.0;   // the sums, and the int32 bins: all bits zero
        return;
    }
    double mx = -INFINITY;
    for (int j = 0; j < N; ++j) mx = lw_s[j] > mx ? lw_s[j] : mx;
    if (tid < N) w_s[tid] = alive ? exp(lw_s[tid] - mx) : 0.0;
    __syncthreads();
    double W = 0.0;
    for (int j = 0; j < N; ++j) W += w_s[j];
    const double my_w = tid < N ? w_s[tid] / W : 0.0;
    __syncthreads();   // every thread has read the exponentials
    if (tid < N) w_s[tid] = my_w;
    __syncthreads();
    double q = 0.0;
    for (int j = 0; j < N; ++j) q = fma(w_s[j], w_s[j], q);
    const double cq = P.unbiased ? 1.0 - q : 1.0;

    const int j0 = wave * 16;
    const bool active = j0 < N;                 // uniform over the wave
    const int jm = j0 + li;
    const int64_t m = ((int64_t)b * N + (jm < N ? jm : 0)) * P.P + patch;
    double acc_sum = 0.0;                       // threads 0 .. 7: the field's running sums

    int gsel = 0;   // the group that holds the field: the entry point has checked that exactly one does
    for (int gi = 1; gi < L.n_groups; ++gi) gsel = (fg >= L.g[gi].field0 && fg < L.g[gi].field0 + L.g[gi].n_fields) ? gi : gsel;
    {
        const SeaDecodeMseGroup& G = L.g[gsel];
        const int j = fg - G.field0;   // the field inside its group
        const __bf16* H = static_cast<const __bf16*>(G.H);
        const __bf16* W2 = static_cast<const __bf16*>(G.W2);
        uint4 hf[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int s = ks * 32 + 8 * lg;
            // a row at or beyond N repeats member 0's: its values are stored to V and never read.  The k-step that straddles S loads column 0 where
            // s >= S and selects zeros (the tile image is zero there, but 0 * NaN is not)
            if (ks * 32 + 32 <= S) {
                hf[ks] = *reinterpret_cast<const uint4*>(H + m * G.ldh + s);
            } else {
                const uint4 v = *reinterpret_cast<const uint4*>(H + m * G.ldh + (s < S ? s : 0));
                hf[ks] = s < S ? v : make_uint4(0u, 0u, 0u, 0u);
            }
        }
        const int n_tiles = te - tb, t0 = j * tpf + tb;   // this chunk's tiles among the group's
        uint4 wr[NCH];
        dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t0, tid);
        dm_store_tile<SP, NT>(wr, smem, tid);
        __syncthreads();

        for (int t = 0; t < n_tiles; ++t) {
            const char* buf = smem + (t & 1) * TILE;
            const int cb = (tb + t) * DM_TC;

            // a: the columns' weights and readings; decode into the value image
            if (tid < DM_TC) {
                const int c = cb + tid;
                float w = 0.f;
                if (c < lim) {
                    const float pf = P.prec_field != nullptr ? P.prec_field[fg] : 1.f;
                    const float pm = P.prec != nullptr ? P.prec[(int64_t)bp * P.ld_prow + (int64_t)fg * P.ld_pfield + c] : 1.f;
                    w = mul1(pf > 0.f ? pf : 0.f, pm > 0.f ? pm : 0.f);
                }
                const bool on = w > 0.f;   // false for NaN
                pv_s[tid] = on ? w : 0.f;
                y_s[tid] = on ? P.obs[(int64_t)bp * P.ld_row + (int64_t)fg * P.ld_field + c] : 0.f;
            }
            if (active) {
                f32x4 acc[2][2];
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    const float bv = G.bias[j * Cp + cb + sub * 16 + li];
                    acc[sub][0] = f32x4{bv, bv, bv, bv};
                    acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    if (ks * 32 < S) {
#pragma unroll
                        for (int sub = 0; sub < 2; ++sub) {
                            const uint4 wv = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                            mma16<__bf16>(hf[ks], wv, acc[sub][ks & 1]);
                        }
                    }
                }
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)   // plain C++: the first reader of an MFMA result must be an instruction the compiler sees
                        Vs[(sub * 16 + li) * VP + j0 + 4 * lg + r] = acc[sub][0][r] + acc[sub][1][r];
                }
            }
            __syncthreads();
            if (t + 1 < n_tiles) dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t0 + t + 1, tid);   // in flight behind b

            // b: a column per wave at a time
            for (int cl = wave; cl < DM_TC; cl += NW) {
                const float pv = pv_s[cl];
                if (!(pv > 0.f)) {   // the same word in every lane
                    if (lane == 0) r_s[cl].state = 1;
                    continue;
                }
                const VfReading r = vf_score_wave<V>(Vs + cl * VP, w_s, live_s, N, lane, y_s[cl], pv);
                if (lane == 0) r_s[cl] = r;
            }
            __syncthreads();

            // c: thread k finishes column k
            if (tid < DM_TC) {
                double tm[VF_SUMS];
                const VfReading r = r_s[tid];
                const VfOut o = vf_finish_reading(r, y_s[tid], pv_s[tid], cq, tm);
                if (r.state == 0) atomicAdd(&hist_s[o.rank], 1);   // LDS, integers: the order does not matter; 0 <= rank <= N
                const int c = cb + tid;
                if (c < ld) {
                    const int64_t at = obase + c;
                    if (P.mean != nullptr) P.mean[at] = o.mean;
                    if (P.spread != nullptr) P.spread[at] = o.spread;
                    if (P.crps != nullptr) P.crps[at] = o.crps;
                    if (P.pit != nullptr) P.pit[at] = o.pit;
                    if (P.rank != nullptr) P.rank[at] = o.rank;
                }
#pragma unroll
                for (int i = 0; i < VF_SUMS; ++i) term_s[i][tid] = tm[i];
            }
            if (t + 1 < n_tiles) dm_store_tile<SP, NT>(wr, smem + ((t + 1) & 1) * TILE, tid);
            __syncthreads();

            // d: the field's sums, columns ascending (the next tile's terms are filed two barriers ahead)
            if (tid < VF_SUMS)
                for (int k = 0; k < DM_TC; ++k) acc_sum += term_s[tid][k];
        }
    }
    if (tid < VF_SUMS) wsum[tid] = acc_sum;
    for (int r = tid; r <= N; r += NT) whist[r] = hist_s[r];   // every integer add lies behind the last tile's barrier
}

__global__ __launch_bounds__(256) void member_verify_finish_kernel(const SeaDecodeMemberVerify p, const int chunks, const int words) {
#pragma clang fp reassociate(off)
    const int tid = threadIdx.x, b = blockIdx.x, N = p.members, F = p.n_fields_total, Pn = p.P * chunks;   // (patch, chunk) partials per field
    const double* base = reinterpret_cast<const double*>(p.work) + (int64_t)b * Pn * F * words;
    for (int e = tid; e < F * VF_SUMS; e += 256) {
        const int f = e / VF_SUMS, i = e - f * VF_SUMS;
        double acc = 0.0;
#pragma unroll 8
        for (int pt = 0; pt < Pn; ++pt) acc += base[((int64_t)pt * F + f) * words + i];   // (patch, chunk) ascending
        double* dst = p.sums + ((int64_t)b * F + f) * VF_SUMS + i;
        *dst = p.accumulate ? *dst + acc : acc;
    }
    for (int e = tid; e < F * (N + 1); e += 256) {
        const int f = e / (N + 1), r = e - f * (N + 1);
        int64_t s = 0;
#pragma unroll 8
        for (int pt = 0; pt < Pn; ++pt) s += reinterpret_cast<const int32_t*>(base + ((int64_t)pt * F + f) * words + VF_SUMS)[r];   // integers: any order
        int64_t* dst = p.hist + ((int64_t)b * F + f) * (N + 1) + r;
        *dst = p.accumulate ? *dst + s : s;
    }
}

template <int SP, int V>
static void member_verify_launch(const MemberVerifyLaunch& L, dim3 grid, hipStream_t s) {
    constexpr int lds = mv_lds_bytes<SP>();
    static bool set_on[64] = {false};   // per device: the dynamic part is 100 kB at SP = 640, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_member_verify_kernel<SP, V>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_member_verify_kernel<SP, V><<<grid, dim3(MV_NT), lds, s>>>(L);
    sea_note_form("decode.member_verify", SP, lds);
}

template <int V>
static void member_verify_dispatch(const MemberVerifyLaunch& L, dim3 grid, hipStream_t s) {
    if (L.p.S <= 128) member_verify_launch<128, V>(L, grid, s);
    else if (L.p.S <= 256) member_verify_launch<256, V>(L, grid, s);
    else if (L.p.S <= 384) member_verify_launch<384, V>(L, grid, s);
    else if (L.p.S <= 512) member_verify_launch<512, V>(L, grid, s);
    else member_verify_launch<640, V>(L, grid, s);
}

extern "C" int64_t sea_decode_member_verify_ws_bytes(int B, int P, int n_fields_total, int members, int Cp) {
    if (B < 1 || B > 65535 || P < 1 || n_fields_total < 1 || members < 1 || members > VF_MAX_N || Cp < 32 || Cp % 32) return -1;
    return (int64_t)B * P * mv_chunks(Cp) * n_fields_total * mv_words(members) * 8;
}

extern "C" int sea_decode_member_verify(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberVerify* p, int dtype, void* stream) {
    SEA_REQUIRE(groups != nullptr && p != nullptr, "sea_decode_member_verify: null argument table");
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "sea_decode_member_verify: n_groups=%d outside 1..%d", n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "sea_decode_member_verify: bad dtype %d", dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("sea_decode_member_verify: unsupported: bf16 only (the fp32 decoder composes the decode and sea_ensemble_verify's formulas)");
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeMemberVerify& P = *p;
    SEA_REQUIRE(P.obs != nullptr && P.sums != nullptr && P.hist != nullptr && P.status != nullptr && P.work != nullptr,
                "sea_decode_member_verify: null pointer (obs, sums, hist, status and work are required; prec_field, prec, counts, logw and the maps may be NULL)");
    SEA_REQUIRE(P.M >= 1, "sea_decode_member_verify: M=%d must be positive", P.M);
    SEA_REQUIRE(P.S >= 8 && P.S % 8 == 0, "sea_decode_member_verify: S=%d must be a positive multiple of 8", P.S);
    SEA_REQUIRE(P.Cp >= 32 && P.Cp % 32 == 0, "sea_decode_member_verify: Cp=%d must be a positive multiple of 32", P.Cp);
    SEA_REQUIRE(P.C >= 1 && P.C <= P.Cp, "sea_decode_member_verify: C=%d must lie in 1..Cp=%d", P.C, P.Cp);
    SEA_REQUIRE(P.P >= 1, "sea_decode_member_verify: P=%d must be positive", P.P);
    SEA_REQUIRE(P.members >= 1, "sea_decode_member_verify: members=%d must be positive", P.members);
    SEA_REQUIRE((int64_t)P.M % ((int64_t)P.P * P.members) == 0, "sea_decode_member_verify: M=%d is not a multiple of P * members = %d * %d", P.M, P.P, P.members);
    SEA_REQUIRE(P.n_fields_total >= 1, "sea_decode_member_verify: n_fields_total=%d must be positive", P.n_fields_total);
    SEA_REQUIRE(P.ld_field >= P.C && P.ld_row >= 0, "sea_decode_member_verify: obs strides ld_row=%lld, ld_field=%lld must cover C=%d", (long long)P.ld_row,
                (long long)P.ld_field, P.C);
    SEA_REQUIRE(P.prec == nullptr || (P.ld_pfield >= P.C && P.ld_prow >= 0), "sea_decode_member_verify: prec strides ld_prow=%lld, ld_pfield=%lld must cover C=%d",
                (long long)P.ld_prow, (long long)P.ld_pfield, P.C);
    SEA_REQUIRE((P.mean == nullptr && P.spread == nullptr && P.crps == nullptr && P.pit == nullptr && P.rank == nullptr) || P.ld_out >= P.C,
                "sea_decode_member_verify: ld_out=%lld must cover C=%d", (long long)P.ld_out, P.C);
    SEA_REQUIRE((P.unbiased == 0 || P.unbiased == 1) && (P.accumulate == 0 || P.accumulate == 1), "sea_decode_member_verify: unbiased=%d and accumulate=%d must be 0 or 1",
                P.unbiased, P.accumulate);
    SEA_REQUIRE(sea_aligned4(P.obs) && sea_aligned4(P.prec_field) && sea_aligned4(P.prec) && sea_aligned4(P.counts) && sea_aligned4(P.logw) && sea_aligned4(P.mean) &&
                    sea_aligned4(P.spread) && sea_aligned4(P.crps) && sea_aligned4(P.pit) && sea_aligned4(P.rank) && sea_aligned4(P.status) &&
                    (reinterpret_cast<uintptr_t>(P.sums) & 7u) == 0 && (reinterpret_cast<uintptr_t>(P.hist) & 7u) == 0 && (reinterpret_cast<uintptr_t>(P.work) & 7u) == 0,
                "sea_decode_member_verify: misaligned pointer (f32 and int32 buffers need 4 bytes; sums, hist and work 8)");
    int64_t covered = 0;
    for (int g = 0; g < n_groups; ++g) {
        const SeaDecodeMseGroup& G = groups[g];
        SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr, "sea_decode_member_verify: group %d: null pointer", g);
        SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias), "sea_decode_member_verify: group %d: pointers must be 16-byte aligned", g);
        SEA_REQUIRE(G.ldh >= P.S && G.ldh % 8 == 0 && G.ldw >= P.S && G.ldw % 8 == 0,
                    "sea_decode_member_verify: group %d: row strides ldh=%d ldw=%d must cover S=%d and be multiples of 8", g, G.ldh, G.ldw, P.S);
        SEA_REQUIRE(G.n_fields >= 1 && G.field0 >= 0 && (int64_t)G.field0 + G.n_fields <= P.n_fields_total,
                    "sea_decode_member_verify: group %d: n_fields=%d, field0=%d outside the %d fields", g, G.n_fields, G.field0, P.n_fields_total);
        SEA_REQUIRE((int64_t)G.n_fields * P.Cp <= 0x7fffffffLL / 2, "sea_decode_member_verify: group %d: too many output columns", g);
        for (int h = 0; h < g; ++h)
            SEA_REQUIRE(G.field0 >= groups[h].field0 + groups[h].n_fields || groups[h].field0 >= G.field0 + G.n_fields,
                        "sea_decode_member_verify: group %d: its fields overlap those of group %d (a cell is scored once)", g, h);
        covered += G.n_fields;
    }
    SEA_REQUIRE(covered == P.n_fields_total, "sea_decode_member_verify: the groups cover %lld of the %d fields (every field needs exactly one group)", (long long)covered,
                P.n_fields_total);
    if (P.S > 640) {
        sea_set_error("sea_decode_member_verify: unsupported: hidden width S=%d above 640", P.S);
        return SEA_EUNSUPPORTED;
    }
    if (P.members > VF_MAX_N) {
        sea_set_error("sea_decode_member_verify: unsupported: members=%d above %d", P.members, VF_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    const int64_t BP = (int64_t)P.M / P.members;   // (history, patch) pairs
    const int64_t B = BP / P.P;
    SEA_REQUIRE(BP <= 0x7fffffffLL && B <= 65535, "sea_decode_member_verify: %lld histories; a launch carries up to 65535", (long long)B);
    SEA_REQUIRE((int64_t)P.n_fields_total * mv_words(P.members) <= 0x7fffffffLL && (int64_t)P.n_fields_total * (P.members + 1) <= 0x7fffffffLL,
                "sea_decode_member_verify: too many fields");
    const int64_t need = sea_decode_member_verify_ws_bytes((int)B, P.P, P.n_fields_total, P.members, P.Cp);
    SEA_REQUIRE(P.work_bytes >= need,
                "sea_decode_member_verify: work_bytes=%lld below the %lld that sea_decode_member_verify_ws_bytes(B=%d, P=%d, n_fields_total=%d, members=%d, Cp=%d) asks for",
                (long long)P.work_bytes, (long long)need, (int)B, P.P, P.n_fields_total, P.members, P.Cp);
    SEA_REQUIRE((int64_t)P.P * mv_chunks(P.Cp) <= 0x7fffffffLL && mv_chunks(P.Cp) <= 65535, "sea_decode_member_verify: Cp=%d has too many column chunks", P.Cp);

    MemberVerifyLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    L.n_groups = n_groups;
    L.words = (int)mv_words(P.members);
    hipStream_t s = static_cast<hipStream_t>(stream);
    SEA_REQUIRE(P.n_fields_total <= 65535, "sea_decode_member_verify: n_fields_total=%d above 65535 (a grid dimension)", P.n_fields_total);
    const dim3 grid((unsigned)BP, (unsigned)P.n_fields_total, (unsigned)mv_chunks(P.Cp));
    if (P.members <= 64) member_verify_dispatch<1>(L, grid, s);
    else member_verify_dispatch<2>(L, grid, s);
    member_verify_finish_kernel<<<dim3((unsigned)B), dim3(256), 0, s>>>(P, mv_chunks(P.Cp), L.words);
    SEA_CHECK_LAUNCH("sea_decode_member_verify");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_member_quantiles: weighted quantile maps and exceedance-probability maps of an ensemble's decoded fields (include/sea_hip.h states the
// definitions).  ONE launch with decode_member_verify_kernel's grid — a workgroup of 8 waves per (history, patch, field, chunk of MV_CHUNK tiles) —
// and its decode, line for line: dm_load_tile / dm_store_tile, the bias in the accumulator, the acc0 + acc1 store to V[column][member] at the
// 129-float stride.  A cell decoded here has the bits of the cell sea_decode_member_verify scores.  Per tile:
//   a  the waves decode their 16 members and write the value image;
//   b  wave w reads out the columns w, w + 8, w + 16, w + 24 (qs_column_wave, quantile_select.hpp: the walk for the weight below every member only
//      when the launch has levels; per level a select and an f32 wave-min; per threshold one fp64 butterfly); lane 0 files the column's
//      n_levels + n_thr results in res_s; a column at or beyond the patch's valid count is passed over;
//   c  thread k stores column k of every map — one writer per element, 128-byte segments — while the next tile of W2 goes to its LDS image.
// Three barriers per tile.  Columns at or beyond the walked tiles are filled with 0 before the walk.  Nothing is reduced across workgroups: there is no
// finish launch, no workspace and no atomic of any kind.
// LDS at SP = 640: 2 x 41984 (W2 images) + 16512 (V) dynamic, 3.8 kB static (weights, live flags, results, thresholds): 104 kB, one workgroup per CU.
struct MemberQuantLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeMemberQuantiles p;
    int n_groups;
};

// The decode of decode_member_quantiles_kernel and decode_member_brier_kernel, one copy for both: a cell decoded by either has the same bits.
// mq_load_row: a lane's k-slices of its member's hidden row.  A row at or beyond N repeats member 0's: its values are stored to V and never read.  The
// k-step that straddles S loads column 0 where s >= S and selects zeros (the tile image is zero there, but 0 * NaN is not).
template <int SP>
__device__ __forceinline__ void mq_load_row(uint4 (&hf)[SP / 32], const __bf16* hrow, const int S, const int lg) {
#pragma unroll
    for (int ks = 0; ks < SP / 32; ++ks) {
        const int s = ks * 32 + 8 * lg;
        if (ks * 32 + 32 <= S) {
            hf[ks] = *reinterpret_cast<const uint4*>(hrow + s);
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(hrow + (s < S ? s : 0));
            hf[ks] = s < S ? v : make_uint4(0u, 0u, 0u, 0u);
        }
    }
}

// mq_decode_tile: a wave's 16 members times the tile's 32 columns into the value image; bias: the tile's 32 entries; vcol: V + the wave's first member.
template <int SP>
__device__ __forceinline__ void mq_decode_tile(const uint4 (&hf)[SP / 32], const char* buf, const float* bias, const int S, const int li, const int lg, float* vcol) {
    constexpr int PITCH = SP * 2 + DM_PAD;
    f32x4 acc[2][2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
        const float bv = bias[sub * 16 + li];
        acc[sub][0] = f32x4{bv, bv, bv, bv};
        acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ks = 0; ks < SP / 32; ++ks) {
        if (ks * 32 < S) {
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const uint4 wv = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                mma16<__bf16>(hf[ks], wv, acc[sub][ks & 1]);
            }
        }
    }
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int r = 0; r < 4; ++r)   // plain C++: the first reader of an MFMA result must be an instruction the compiler sees
            vcol[(sub * 16 + li) * MV_VP + 4 * lg + r] = acc[sub][0][r] + acc[sub][1][r];
    }
}

template <int SP, int V>
__global__ __launch_bounds__(MV_NT) void decode_member_quantiles_kernel(const MemberQuantLaunch L) {
#pragma clang fp reassociate(off)
    constexpr int NW = MV_NW;
    constexpr int NT = MV_NT;
    constexpr int KS = SP / 32;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    constexpr int VP = MV_VP;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images; the value image [32][VP]
    float* Vs = reinterpret_cast<float*>(smem + 2 * TILE);
    __shared__ double w_s[VF_MAX_N];
    __shared__ int live_s[VF_MAX_N];
    __shared__ float res_s[DM_TC][QS_MAX_OUT];
    __shared__ float thr_s[SEA_QUANTILE_MAX_LEVELS];

    const SeaDecodeMemberQuantiles& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
    const int S = P.S, C = P.C, Cp = P.Cp, N = P.members, F = P.n_fields_total, nl = P.n_levels, nt = P.n_thr;
    const int bp = blockIdx.x, fg = blockIdx.y, ck = blockIdx.z;   // the field and the chunk of its tiles this workgroup reads out
    const int b = bp / P.P, patch = bp - b * P.P;
    const int64_t ld = P.ld;
    const int64_t obase = ((int64_t)bp * F + fg) * ld;

    int lim = C;   // valid columns of this patch: [0, lim) — uniform over the workgroup
    if (P.counts != nullptr) {
        const int cnt = P.counts[patch];
        lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
    }
    const int tpf = (lim + DM_TC - 1) / DM_TC;   // tiles of a field that hold valid columns
    const int tb = ck * MV_CHUNK, te = tpf < tb + MV_CHUNK ? tpf : tb + MV_CHUNK;   // this workgroup's tiles: [tb, te)

    // the weights of the history: a member with w <= 0 or NaN is dead
    int alive = 0;
    if (tid < N) {
        const float wv = P.w != nullptr ? P.w[(int64_t)b * N + tid] : 1.f;
        alive = wv > 0.f ? 1 : 0;   // false for NaN
        w_s[tid] = alive ? (double)wv : 0.0;
        live_s[tid] = alive;
    }
    if (tid < nt) thr_s[tid] = P.thr[(int64_t)tid * F + fg];
    const int n_live = __syncthreads_count(alive);
    const bool empty = n_live == 0;
    if (ck == 0) {   // the columns no tile walks (all of them when the history has no live member or the patch no valid column): 0
        const int c0 = (empty || tpf == 0) ? 0 : tpf * DM_TC;
        for (int64_t c = c0 + tid; c < ld; c += NT) {
            const int64_t at = obase + c;
            for (int k = 0; k < nl; ++k) P.quant[k * P.ld_map + at] = 0.f;
            for (int t = 0; t < nt; ++t) P.exceed[t * P.ld_map + at] = 0.f;
        }
    }
    if (empty || te <= tb) return;   // uniform: nothing to read out in this chunk
    double W = 0.0;
    for (int j = 0; j < N; ++j) W += w_s[j];   // one chain, j ascending; a dead member adds +0

    const int j0 = wave * 16;
    const bool active = j0 < N;                 // uniform over the wave
    const int jm = j0 + li;
    const int64_t m = ((int64_t)b * N + (jm < N ? jm : 0)) * P.P + patch;

    int gsel = 0;   // the group that holds the field: the entry point has checked that exactly one does
    for (int gi = 1; gi < L.n_groups; ++gi) gsel = (fg >= L.g[gi].field0 && fg < L.g[gi].field0 + L.g[gi].n_fields) ? gi : gsel;
    const SeaDecodeMseGroup& G = L.g[gsel];
    const int j = fg - G.field0;   // the field inside its group
    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    uint4 hf[KS];
    mq_load_row<SP>(hf, H + m * G.ldh, S, lg);
    const int n_tiles = te - tb, t0 = j * tpf + tb;   // this chunk's tiles among the group's
    uint4 wr[NCH];
    dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t0, tid);
    dm_store_tile<SP, NT>(wr, smem, tid);
    __syncthreads();

    for (int t = 0; t < n_tiles; ++t) {
        const char* buf = smem + (t & 1) * TILE;
        const int cb = (tb + t) * DM_TC;

        // a: decode into the value image
        if (active) mq_decode_tile<SP>(hf, buf, G.bias + j * Cp + cb, S, li, lg, Vs + j0);
        __syncthreads();
        if (t + 1 < n_tiles) dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t0 + t + 1, tid);   // in flight behind b

        // b: a column per wave at a time
        for (int cl = wave; cl < DM_TC; cl += NW) {
            if (cb + cl >= lim) continue;   // the same word in every lane: a dead column, stage c writes its zeros
            qs_column_wave<V>(Vs + cl * VP, w_s, live_s, N, lane, W, P.level, nl, thr_s, nt, res_s[cl]);
        }
        __syncthreads();

        // c: thread k stores column k of every map
        if (tid < DM_TC) {
            const int c = cb + tid;
            if (c < ld) {
                const int64_t at = obase + c;
                const bool on = c < lim;
                for (int k = 0; k < nl; ++k) P.quant[k * P.ld_map + at] = on ? res_s[tid][k] : 0.f;
                for (int q = 0; q < nt; ++q) P.exceed[q * P.ld_map + at] = on ? res_s[tid][nl + q] : 0.f;
            }
        }
        if (t + 1 < n_tiles) dm_store_tile<SP, NT>(wr, smem + ((t + 1) & 1) * TILE, tid);
        __syncthreads();
    }
}

template <int SP, int V>
static void member_quantiles_launch(const MemberQuantLaunch& L, dim3 grid, hipStream_t s) {
    constexpr int lds = mv_lds_bytes<SP>();
    static bool set_on[64] = {false};   // per device: the dynamic part is 100 kB at SP = 640, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_member_quantiles_kernel<SP, V>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_member_quantiles_kernel<SP, V><<<grid, dim3(MV_NT), lds, s>>>(L);
    sea_note_form("decode.member_quantiles", SP, lds);
}

template <int V>
static void member_quantiles_dispatch(const MemberQuantLaunch& L, dim3 grid, hipStream_t s) {
    if (L.p.S <= 128) member_quantiles_launch<128, V>(L, grid, s);
    else if (L.p.S <= 256) member_quantiles_launch<256, V>(L, grid, s);
    else if (L.p.S <= 384) member_quantiles_launch<384, V>(L, grid, s);
    else if (L.p.S <= 512) member_quantiles_launch<512, V>(L, grid, s);
    else member_quantiles_launch<640, V>(L, grid, s);
}

extern "C" int sea_decode_member_quantiles(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberQuantiles* p, int dtype, void* stream) {
    SEA_REQUIRE(groups != nullptr && p != nullptr, "sea_decode_member_quantiles: null argument table");
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "sea_decode_member_quantiles: n_groups=%d outside 1..%d", n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "sea_decode_member_quantiles: bad dtype %d", dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("sea_decode_member_quantiles: unsupported: bf16 only (the fp32 decoder composes the decode and a sort)");
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeMemberQuantiles& P = *p;
    SEA_REQUIRE(P.n_levels >= 0 && P.n_levels <= SEA_QUANTILE_MAX_LEVELS && P.n_thr >= 0 && P.n_thr <= SEA_QUANTILE_MAX_LEVELS && P.n_levels + P.n_thr >= 1,
                "sea_decode_member_quantiles: n_levels=%d and n_thr=%d must lie in 0..%d and not both be 0", P.n_levels, P.n_thr, SEA_QUANTILE_MAX_LEVELS);
    for (int k = 0; k < P.n_levels; ++k)
        SEA_REQUIRE(P.level[k] >= 0.f && P.level[k] <= 1.f, "sea_decode_member_quantiles: level[%d]=%g must be finite and lie in [0, 1]", k, (double)P.level[k]);
    SEA_REQUIRE((P.n_levels == 0 || P.quant != nullptr) && (P.n_thr == 0 || (P.thr != nullptr && P.exceed != nullptr)),
                "sea_decode_member_quantiles: null pointer (quant is required with levels, thr and exceed with thresholds; w and counts may be NULL)");
    SEA_REQUIRE(P.M >= 1, "sea_decode_member_quantiles: M=%d must be positive", P.M);
    SEA_REQUIRE(P.S >= 8 && P.S % 8 == 0, "sea_decode_member_quantiles: S=%d must be a positive multiple of 8", P.S);
    SEA_REQUIRE(P.Cp >= 32 && P.Cp % 32 == 0, "sea_decode_member_quantiles: Cp=%d must be a positive multiple of 32", P.Cp);
    SEA_REQUIRE(P.C >= 1 && P.C <= P.Cp, "sea_decode_member_quantiles: C=%d must lie in 1..Cp=%d", P.C, P.Cp);
    SEA_REQUIRE(P.P >= 1, "sea_decode_member_quantiles: P=%d must be positive", P.P);
    SEA_REQUIRE(P.members >= 1, "sea_decode_member_quantiles: members=%d must be positive", P.members);
    SEA_REQUIRE((int64_t)P.M % ((int64_t)P.P * P.members) == 0, "sea_decode_member_quantiles: M=%d is not a multiple of P * members = %d * %d", P.M, P.P, P.members);
    SEA_REQUIRE(P.n_fields_total >= 1 && P.n_fields_total <= 65535, "sea_decode_member_quantiles: n_fields_total=%d outside 1..65535 (a grid dimension)", P.n_fields_total);
    const int64_t BP = (int64_t)P.M / P.members;   // (history, patch) pairs
    const int64_t B = BP / P.P;
    SEA_REQUIRE(BP <= 0x7fffffffLL && B <= 65535, "sea_decode_member_quantiles: %lld histories; a launch carries up to 65535", (long long)B);
    SEA_REQUIRE(P.ld >= P.C && P.ld <= 0x7fffffffLL && P.ld_map >= BP * P.n_fields_total * P.ld,
                "sea_decode_member_quantiles: ld=%lld must cover C=%d, and ld_map=%lld a whole map of %lld floats", (long long)P.ld, P.C, (long long)P.ld_map,
                (long long)(BP * P.n_fields_total * P.ld));
    SEA_REQUIRE(sea_aligned4(P.w) && sea_aligned4(P.counts) && sea_aligned4(P.thr) && sea_aligned4(P.quant) && sea_aligned4(P.exceed),
                "sea_decode_member_quantiles: misaligned pointer (f32 and int32 buffers need 4 bytes)");
    int64_t covered = 0;
    for (int g = 0; g < n_groups; ++g) {
        const SeaDecodeMseGroup& G = groups[g];
        SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr, "sea_decode_member_quantiles: group %d: null pointer", g);
        SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias), "sea_decode_member_quantiles: group %d: pointers must be 16-byte aligned", g);
        SEA_REQUIRE(G.ldh >= P.S && G.ldh % 8 == 0 && G.ldw >= P.S && G.ldw % 8 == 0,
                    "sea_decode_member_quantiles: group %d: row strides ldh=%d ldw=%d must cover S=%d and be multiples of 8", g, G.ldh, G.ldw, P.S);
        SEA_REQUIRE(G.n_fields >= 1 && G.field0 >= 0 && (int64_t)G.field0 + G.n_fields <= P.n_fields_total,
                    "sea_decode_member_quantiles: group %d: n_fields=%d, field0=%d outside the %d fields", g, G.n_fields, G.field0, P.n_fields_total);
        SEA_REQUIRE((int64_t)G.n_fields * P.Cp <= 0x7fffffffLL / 2, "sea_decode_member_quantiles: group %d: too many output columns", g);
        for (int h = 0; h < g; ++h)
            SEA_REQUIRE(G.field0 >= groups[h].field0 + groups[h].n_fields || groups[h].field0 >= G.field0 + G.n_fields,
                        "sea_decode_member_quantiles: group %d: its fields overlap those of group %d (a cell is read out once)", g, h);
        covered += G.n_fields;
    }
    SEA_REQUIRE(covered == P.n_fields_total, "sea_decode_member_quantiles: the groups cover %lld of the %d fields (every field needs exactly one group)",
                (long long)covered, P.n_fields_total);
    if (P.S > 640) {
        sea_set_error("sea_decode_member_quantiles: unsupported: hidden width S=%d above 640", P.S);
        return SEA_EUNSUPPORTED;
    }
    if (P.members > VF_MAX_N) {
        sea_set_error("sea_decode_member_quantiles: unsupported: members=%d above %d", P.members, VF_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    SEA_REQUIRE(mv_chunks(P.Cp) <= 65535, "sea_decode_member_quantiles: Cp=%d has too many column chunks", P.Cp);

    MemberQuantLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    L.n_groups = n_groups;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)BP, (unsigned)P.n_fields_total, (unsigned)mv_chunks(P.Cp));
    if (P.members <= 64) member_quantiles_dispatch<1>(L, grid, s);
    else member_quantiles_dispatch<2>(L, grid, s);
    SEA_CHECK_LAUNCH("sea_decode_member_quantiles");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_member_brier: the threshold scores of an ensemble against a DENSE observation of the decoded fields — Brier sums, the histograms of the
// reliability diagram and the hit counts of the ROC (include/sea_hip.h states the definitions).  Launch 1 is decode_member_quantiles_kernel in its
// thresholds-only form — its grid, mq_load_row / mq_decode_tile, the [column][member] value image — crossed with decode_member_verify_kernel's reads of
// obs, prec_field, prec and counts and its live / dead / bad classification.  Per tile:
//   a  threads 0 .. 31 form the columns' weights (decode_member_verify_kernel's selects) and read obs where the weight is positive; the waves decode;
//   b  wave w scores the columns w, w + 8, w + 16, w + 24 (bs_column_wave, brier_score.hpp: per threshold one fp64 butterfly and two ballots);
//   c  thread (k, t), k + 32 t, finishes threshold t of column k: the two maps — one writer per element, 128-byte segments —, the five terms, and the
//      integer adds to the LDS histograms; the next tile of W2 goes to its LDS image meanwhile;
//   d  thread (t, i) adds the tile's terms in ascending column order onto its running fp64 sum.
// Three barriers per tile.  member_brier_finish_kernel: one workgroup per (history, field, threshold) adds its partials in ascending (patch, chunk) order.
// LDS at SP = 640: 2 x 41984 (W2 images) + 16512 (V) dynamic, 24 kB static (weights, cells, terms, histograms at their maxima): 125 kB of the CU's 160.
struct MemberBrierLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeMemberBrier p;
    int n_groups;
    int words;   // 8-byte words per (history, patch, chunk, field) of the workspace
};

template <int SP, int V>
__global__ __launch_bounds__(MV_NT) void decode_member_brier_kernel(const MemberBrierLaunch L) {
#pragma clang fp reassociate(off)
    constexpr int NW = MV_NW;
    constexpr int NT = MV_NT;
    constexpr int KS = SP / 32;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    constexpr int VP = MV_VP;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    static_assert(DM_TC * BS_MAX_T <= NT, "a thread per (column, threshold)");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images; the value image [32][VP]
    float* Vs = reinterpret_cast<float*>(smem + 2 * TILE);
    __shared__ double lw_s[VF_MAX_N], w_s[VF_MAX_N];
    __shared__ int live_s[VF_MAX_N];
    __shared__ BsCell cell_s[DM_TC];
    __shared__ double term_s[BS_MAX_T * BS_SUMS][DM_TC];
    __shared__ int hist_s[2 * BS_MAX_T * (VF_MAX_N + 1)];   // [hist | hits][t][m] at the call's T and N
    __shared__ float y_s[DM_TC], pv_s[DM_TC], thr_s[BS_MAX_T];

    const SeaDecodeMemberBrier& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
    const int S = P.S, C = P.C, Cp = P.Cp, N = P.members, F = P.n_fields_total, T = P.n_thr, words = L.words;
    const int bp = blockIdx.x, fg = blockIdx.y, ck = blockIdx.z, Q = gridDim.z;
    const int b = bp / P.P, patch = bp - b * P.P;
    const int64_t ld = P.ld_out;
    const int64_t obase = ((int64_t)bp * F + fg) * ld;
    const int nb = T * (N + 1);
    double* const wsum = reinterpret_cast<double*>(P.work) + (((int64_t)bp * Q + ck) * F + fg) * words;
    int32_t* const whist = reinterpret_cast<int32_t*>(wsum + T * BS_SUMS);

    int lim = C;   // valid columns of this patch: [0, lim) — uniform over the workgroup
    if (P.counts != nullptr) {
        const int cnt = P.counts[patch];
        lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
    }
    const int tpf = (lim + DM_TC - 1) / DM_TC;   // tiles of a field that hold valid columns
    const int tb = ck * MV_CHUNK, te = tpf < tb + MV_CHUNK ? tpf : tb + MV_CHUNK;   // this workgroup's tiles: [tb, te)

    for (int r = tid; r < 2 * nb; r += NT) hist_s[r] = 0;
    if (tid < T) thr_s[tid] = P.thr[(int64_t)tid * F + fg];
    double W;
    const int n_live = bs_history_weights(P.logw, b, N, tid, lw_s, w_s, live_s, W);   // two barriers: hist_s and thr_s are set behind them
    const bool unscored = n_live < 0;
    if (patch == 0 && fg == 0 && ck == 0 && tid == 0) P.status[b] = n_live;
    if (ck == 0 && (P.prob != nullptr || P.brier != nullptr)) {   // the columns no tile walks (all of them when the history is not scored or the patch has no valid column): 0
        const int c0 = (unscored || tpf == 0) ? 0 : tpf * DM_TC;
        for (int64_t c = c0 + tid; c < ld; c += NT) {
            const int64_t at = obase + c;
            for (int t = 0; t < T; ++t) {
                if (P.prob != nullptr) P.prob[t * P.ld_map + at] = 0.f;
                if (P.brier != nullptr) P.brier[t * P.ld_map + at] = 0.f;
            }
        }
    }
    if (unscored || te <= tb) {   // uniform: nothing to score in this chunk
        for (int e = tid; e < words; e += NT) wsum[e] = 0.0;   // the sums, and the int32 bins: all bits zero
        return;
    }

    const int j0 = wave * 16;
    const bool active = j0 < N;                 // uniform over the wave
    const int jm = j0 + li;
    const int64_t m = ((int64_t)b * N + (jm < N ? jm : 0)) * P.P + patch;
    double acc_sum = 0.0;                       // threads 0 .. 5 T - 1: the field's running sums

    int gsel = 0;   // the group that holds the field: the entry point has checked that exactly one does
    for (int gi = 1; gi < L.n_groups; ++gi) gsel = (fg >= L.g[gi].field0 && fg < L.g[gi].field0 + L.g[gi].n_fields) ? gi : gsel;
    const SeaDecodeMseGroup& G = L.g[gsel];
    const int j = fg - G.field0;   // the field inside its group
    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    uint4 hf[KS];
    mq_load_row<SP>(hf, H + m * G.ldh, S, lg);
    const int n_tiles = te - tb, t0 = j * tpf + tb;   // this chunk's tiles among the group's
    uint4 wr[NCH];
    dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t0, tid);
    dm_store_tile<SP, NT>(wr, smem, tid);
    __syncthreads();

    for (int t = 0; t < n_tiles; ++t) {
        const char* buf = smem + (t & 1) * TILE;
        const int cb = (tb + t) * DM_TC;

        // a: the columns' weights and readings (decode_member_verify_kernel's); decode into the value image
        if (tid < DM_TC) {
            const int c = cb + tid;
            float w = 0.f;
            if (c < lim) {
                const float pf = P.prec_field != nullptr ? P.prec_field[fg] : 1.f;
                const float pm = P.prec != nullptr ? P.prec[(int64_t)bp * P.ld_prow + (int64_t)fg * P.ld_pfield + c] : 1.f;
                w = mul1(pf > 0.f ? pf : 0.f, pm > 0.f ? pm : 0.f);
            }
            const bool on = w > 0.f;   // false for NaN
            pv_s[tid] = on ? w : 0.f;
            y_s[tid] = on ? P.obs[(int64_t)bp * P.ld_row + (int64_t)fg * P.ld_field + c] : 0.f;
        }
        if (active) mq_decode_tile<SP>(hf, buf, G.bias + j * Cp + cb, S, li, lg, Vs + j0);
        __syncthreads();
        if (t + 1 < n_tiles) dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t0 + t + 1, tid);   // in flight behind b

        // b: a column per wave at a time
        for (int cl = wave; cl < DM_TC; cl += NW) {
            const float pv = pv_s[cl];
            if (!(pv > 0.f)) {   // the same word in every lane
                if (lane == 0) cell_s[cl].state = 1;
                continue;
            }
            bs_column_wave<V>(Vs + cl * VP, w_s, live_s, N, lane, W, y_s[cl], pv, thr_s, T, &cell_s[cl]);
        }
        __syncthreads();

        // c: thread (k, q) finishes threshold q of column k
        if (tid < DM_TC * T) {
            const int k = tid & (DM_TC - 1), q = tid / DM_TC;
            double tm[BS_SUMS];
            const BsOut o = bs_finish_cell(cell_s[k], q, y_s[k], thr_s[q], tm);
            if (o.m >= 0) {   // LDS, integers: the order does not matter; 0 <= m <= N
                atomicAdd(&hist_s[q * (N + 1) + o.m], 1);
                if (o.o) atomicAdd(&hist_s[nb + q * (N + 1) + o.m], 1);
            }
            const int c = cb + k;
            if (c < ld) {
                const int64_t at = q * P.ld_map + obase + c;
                if (P.prob != nullptr) P.prob[at] = o.prob;
                if (P.brier != nullptr) P.brier[at] = o.brier;
            }
#pragma unroll
            for (int i = 0; i < BS_SUMS; ++i) term_s[q * BS_SUMS + i][k] = tm[i];
        }
        if (t + 1 < n_tiles) dm_store_tile<SP, NT>(wr, smem + ((t + 1) & 1) * TILE, tid);
        __syncthreads();

        // d: the field's sums, columns ascending (the next tile's terms are filed two barriers ahead)
        if (tid < T * BS_SUMS)
            for (int k = 0; k < DM_TC; ++k) acc_sum += term_s[tid][k];
    }
    if (tid < T * BS_SUMS) wsum[tid] = acc_sum;
    for (int r = tid; r < 2 * nb; r += NT) whist[r] = hist_s[r];   // every integer add lies behind the last tile's barrier
}

__global__ __launch_bounds__(256) void member_brier_finish_kernel(const SeaDecodeMemberBrier p, const int chunks, const int words) {
    const int b = blockIdx.x, N = p.members, F = p.n_fields_total, T = p.n_thr, Pn = p.P * chunks;   // (patch, chunk) partials per field
    const int f = blockIdx.y / T, t = blockIdx.y - f * T;                                             // a workgroup per (history, field, threshold)
    const double* part = reinterpret_cast<const double*>(p.work) + ((int64_t)b * Pn * F + f) * words;
    const int64_t o = ((int64_t)b * F + f) * T + t;
    bs_finish_threshold(part, Pn, (int64_t)F * words, T, N, t, p.sums + o * BS_SUMS, p.hist + o * (N + 1), p.hits + o * (N + 1), p.accumulate, threadIdx.x, 256);
}

template <int SP, int V>
static void member_brier_launch(const MemberBrierLaunch& L, dim3 grid, hipStream_t s) {
    constexpr int lds = mv_lds_bytes<SP>();
    static bool set_on[64] = {false};   // per device: the dynamic part is 100 kB at SP = 640, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_member_brier_kernel<SP, V>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_member_brier_kernel<SP, V><<<grid, dim3(MV_NT), lds, s>>>(L);
    sea_note_form("decode.member_brier", SP, lds);
}

template <int V>
static void member_brier_dispatch(const MemberBrierLaunch& L, dim3 grid, hipStream_t s) {
    if (L.p.S <= 128) member_brier_launch<128, V>(L, grid, s);
    else if (L.p.S <= 256) member_brier_launch<256, V>(L, grid, s);
    else if (L.p.S <= 384) member_brier_launch<384, V>(L, grid, s);
    else if (L.p.S <= 512) member_brier_launch<512, V>(L, grid, s);
    else member_brier_launch<640, V>(L, grid, s);
}

extern "C" int64_t sea_decode_member_brier_ws_bytes(int B, int P, int n_fields_total, int members, int Cp, int n_thr) {
    if (B < 1 || B > 65535 || P < 1 || n_fields_total < 1 || members < 1 || members > VF_MAX_N || Cp < 32 || Cp % 32 || n_thr < 1 || n_thr > BS_MAX_T) return -1;
    return (int64_t)B * P * mv_chunks(Cp) * n_fields_total * bs_words(n_thr, members) * 8;
}

extern "C" int sea_decode_member_brier(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberBrier* p, int dtype, void* stream) {
    SEA_REQUIRE(groups != nullptr && p != nullptr, "sea_decode_member_brier: null argument table");
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "sea_decode_member_brier: n_groups=%d outside 1..%d", n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "sea_decode_member_brier: bad dtype %d", dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("sea_decode_member_brier: unsupported: bf16 only (the fp32 decoder composes the decode and the formulas)");
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeMemberBrier& P = *p;
    SEA_REQUIRE(P.obs != nullptr && P.thr != nullptr && P.sums != nullptr && P.hist != nullptr && P.hits != nullptr && P.status != nullptr && P.work != nullptr,
                "sea_decode_member_brier: null pointer (obs, thr, sums, hist, hits, status and work are required; prec_field, prec, counts, logw and the maps may be NULL)");
    SEA_REQUIRE(P.n_thr >= 1 && P.n_thr <= BS_MAX_T, "sea_decode_member_brier: n_thr=%d outside 1..%d", P.n_thr, BS_MAX_T);
    SEA_REQUIRE(P.M >= 1, "sea_decode_member_brier: M=%d must be positive", P.M);
    SEA_REQUIRE(P.S >= 8 && P.S % 8 == 0, "sea_decode_member_brier: S=%d must be a positive multiple of 8", P.S);
    SEA_REQUIRE(P.Cp >= 32 && P.Cp % 32 == 0, "sea_decode_member_brier: Cp=%d must be a positive multiple of 32", P.Cp);
    SEA_REQUIRE(P.C >= 1 && P.C <= P.Cp, "sea_decode_member_brier: C=%d must lie in 1..Cp=%d", P.C, P.Cp);
    SEA_REQUIRE(P.P >= 1, "sea_decode_member_brier: P=%d must be positive", P.P);
    SEA_REQUIRE(P.members >= 1, "sea_decode_member_brier: members=%d must be positive", P.members);
    SEA_REQUIRE((int64_t)P.M % ((int64_t)P.P * P.members) == 0, "sea_decode_member_brier: M=%d is not a multiple of P * members = %d * %d", P.M, P.P, P.members);
    SEA_REQUIRE(P.n_fields_total >= 1 && P.n_fields_total <= 65535 / BS_MAX_T, "sea_decode_member_brier: n_fields_total=%d outside 1..%d (a grid dimension)", P.n_fields_total,
                65535 / BS_MAX_T);
    SEA_REQUIRE(P.ld_field >= P.C && P.ld_row >= 0, "sea_decode_member_brier: obs strides ld_row=%lld, ld_field=%lld must cover C=%d", (long long)P.ld_row,
                (long long)P.ld_field, P.C);
    SEA_REQUIRE(P.prec == nullptr || (P.ld_pfield >= P.C && P.ld_prow >= 0), "sea_decode_member_brier: prec strides ld_prow=%lld, ld_pfield=%lld must cover C=%d",
                (long long)P.ld_prow, (long long)P.ld_pfield, P.C);
    const int64_t BP = (int64_t)P.M / P.members;   // (history, patch) pairs
    const int64_t B = BP / P.P;
    SEA_REQUIRE(BP <= 0x7fffffffLL && B <= 65535, "sea_decode_member_brier: %lld histories; a launch carries up to 65535", (long long)B);
    SEA_REQUIRE((P.prob == nullptr && P.brier == nullptr) || (P.ld_out >= P.C && P.ld_out <= 0x7fffffffLL && P.ld_map >= BP * P.n_fields_total * P.ld_out),
                "sea_decode_member_brier: ld_out=%lld must cover C=%d, and ld_map=%lld a whole map", (long long)P.ld_out, P.C, (long long)P.ld_map);
    SEA_REQUIRE(P.accumulate == 0 || P.accumulate == 1, "sea_decode_member_brier: accumulate=%d must be 0 or 1", P.accumulate);
    SEA_REQUIRE(sea_aligned4(P.obs) && sea_aligned4(P.prec_field) && sea_aligned4(P.prec) && sea_aligned4(P.counts) && sea_aligned4(P.logw) && sea_aligned4(P.thr) &&
                    sea_aligned4(P.prob) && sea_aligned4(P.brier) && sea_aligned4(P.status) && (reinterpret_cast<uintptr_t>(P.sums) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(P.hist) & 7u) == 0 && (reinterpret_cast<uintptr_t>(P.hits) & 7u) == 0 && (reinterpret_cast<uintptr_t>(P.work) & 7u) == 0,
                "sea_decode_member_brier: misaligned pointer (f32 and int32 buffers need 4 bytes; sums, hist, hits and work 8)");
    int64_t covered = 0;
    for (int g = 0; g < n_groups; ++g) {
        const SeaDecodeMseGroup& G = groups[g];
        SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr, "sea_decode_member_brier: group %d: null pointer", g);
        SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias), "sea_decode_member_brier: group %d: pointers must be 16-byte aligned", g);
        SEA_REQUIRE(G.ldh >= P.S && G.ldh % 8 == 0 && G.ldw >= P.S && G.ldw % 8 == 0,
                    "sea_decode_member_brier: group %d: row strides ldh=%d ldw=%d must cover S=%d and be multiples of 8", g, G.ldh, G.ldw, P.S);
        SEA_REQUIRE(G.n_fields >= 1 && G.field0 >= 0 && (int64_t)G.field0 + G.n_fields <= P.n_fields_total,
                    "sea_decode_member_brier: group %d: n_fields=%d, field0=%d outside the %d fields", g, G.n_fields, G.field0, P.n_fields_total);
        SEA_REQUIRE((int64_t)G.n_fields * P.Cp <= 0x7fffffffLL / 2, "sea_decode_member_brier: group %d: too many output columns", g);
        for (int h = 0; h < g; ++h)
            SEA_REQUIRE(G.field0 >= groups[h].field0 + groups[h].n_fields || groups[h].field0 >= G.field0 + G.n_fields,
                        "sea_decode_member_brier: group %d: its fields overlap those of group %d (a cell is scored once)", g, h);
        covered += G.n_fields;
    }
    SEA_REQUIRE(covered == P.n_fields_total, "sea_decode_member_brier: the groups cover %lld of the %d fields (every field needs exactly one group)", (long long)covered,
                P.n_fields_total);
    if (P.S > 640) {
        sea_set_error("sea_decode_member_brier: unsupported: hidden width S=%d above 640", P.S);
        return SEA_EUNSUPPORTED;
    }
    if (P.members > VF_MAX_N) {
        sea_set_error("sea_decode_member_brier: unsupported: members=%d above %d", P.members, VF_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    SEA_REQUIRE((int64_t)P.n_fields_total * bs_words(P.n_thr, P.members) <= 0x7fffffffLL, "sea_decode_member_brier: too many fields");
    const int64_t need = sea_decode_member_brier_ws_bytes((int)B, P.P, P.n_fields_total, P.members, P.Cp, P.n_thr);
    SEA_REQUIRE(P.work_bytes >= need,
                "sea_decode_member_brier: work_bytes=%lld below the %lld that sea_decode_member_brier_ws_bytes(B=%d, P=%d, n_fields_total=%d, members=%d, Cp=%d, n_thr=%d) asks for",
                (long long)P.work_bytes, (long long)need, (int)B, P.P, P.n_fields_total, P.members, P.Cp, P.n_thr);
    SEA_REQUIRE((int64_t)P.P * mv_chunks(P.Cp) <= 0x7fffffffLL && mv_chunks(P.Cp) <= 65535, "sea_decode_member_brier: Cp=%d has too many column chunks", P.Cp);

    MemberBrierLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    L.n_groups = n_groups;
    L.words = (int)bs_words(P.n_thr, P.members);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)BP, (unsigned)P.n_fields_total, (unsigned)mv_chunks(P.Cp));
    if (P.members <= 64) member_brier_dispatch<1>(L, grid, s);
    else member_brier_dispatch<2>(L, grid, s);
    member_brier_finish_kernel<<<dim3((unsigned)B, (unsigned)(P.n_fields_total * P.n_thr)), dim3(256), 0, s>>>(P, mv_chunks(P.Cp), L.words);
    SEA_CHECK_LAUNCH("sea_decode_member_brier");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_derived_quantiles / sea_decode_derived_brier: the two read-outs above for DERIVED fields — x = |(a', b')|, (a'^2 + b'^2) / 2 or a' - b'
// of two source fields of ONE decoder group, per member and cell (include/sea_hip.h states the definitions).  The kernels are
// decode_member_quantiles_kernel and decode_member_brier_kernel with grid.y = n_derived and stage a replaced by a two-source decode
// (mq_decode_pair_tile): the W2 tiles of source a and of source b go through the same two LDS images — a's tile in the first, b's in the second: the
// stream a_0, b_0, a_1, b_1, ... — the hidden rows are loaded once, a's tile is decoded into 8 registers (mq_decode_regs: mq_decode_tile's sums in
// its order), b's tile on top of them, the op is applied per element in single-rounded f32 (mul1 / add1; dv_sqrt_rn) and x goes to V[column][member].
// Both tiles of the next step are fetched behind stage b (two staging sets) and stored in stage c: three barriers per tile as before, LDS at
// mv_lds_bytes<SP>().  Everything behind the value image is the member kernels' code (qs_column_wave, bs_column_wave, bs_finish_cell,
// member_brier_finish_kernel), indexed by derived field.
struct DerivedTable {
    SeaDerivedField d[SEA_DERIVED_MAX];
    int gsel[SEA_DERIVED_MAX];   // the group that holds both sources of derived field i (the entry point has resolved it)
    int n_derived;
};
struct DerivedQuantLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeMemberQuantiles p;
    DerivedTable t;
};
struct DerivedBrierLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeMemberBrier p;
    DerivedTable t;
    int words;   // 8-byte words per (history, patch, chunk, derived field) of the workspace
};

// The correctly rounded f32 square root.  The build's -ffast-math turns sqrtf (and __fsqrt_rn) into the bare v_sqrt_f32, an approximation.  So: the
// hardware root s; one Newton step s + (x - s s) / (2 s) with the residual from ONE fma (exact this close to the root) and the quotient from
// v_rcp_f32, so that what follows does not lean on the last bits of the hardware root; then the choice among s and its two neighbours by the sign of
// the fma residuals x - s_down s and x - s_up s (the compiler's own IEEE lowering of llvm.sqrt.f32, written out), which is the rounded root for any
// start within 1 ulp.  Arguments below 2^-96 are scaled by 2^32 (the root by 2^-16) so that no residual is flushed; +-0 and +inf return themselves,
// a negative argument or NaN gives NaN.  (tests/test_derived_fields_gpu.py: equal bits with the root of float64 rounded once.)
__device__ __forceinline__ float dv_sqrt_rn(const float x) {
    const bool small = x < 0x1p-96f;
    const float xs = small ? mul1(x, 0x1p+32f) : x;
    float s = __builtin_amdgcn_sqrtf(xs);
    s = fma1(fma1(-s, s, xs), mul1(0.5f, __builtin_amdgcn_rcpf(s)), s);
    const float sd = __int_as_float(__float_as_int(s) - 1), su = __int_as_float(__float_as_int(s) + 1);
    const float dd = fma1(-sd, s, xs), du = fma1(-su, s, xs);
    s = dd <= 0.f ? sd : s;
    s = du > 0.f ? su : s;
    s = small ? mul1(s, 0x1p-16f) : s;
    return (xs == 0.f || xs == __builtin_inff()) ? xs : s;
}

// One member's derived value at one cell from the two decoded source values: every operation rounded once.
__device__ __forceinline__ float dv_value(const int op, const float ya, const float yb, const float sa, const float ha, const float sb, const float hb) {
    const float a = add1(mul1(ya, sa), ha), b = add1(mul1(yb, sb), hb);
    if (op == SEA_DERIVED_DIFFERENCE) return add1(a, -b);
    const float q = add1(mul1(a, a), mul1(b, b));
    return op == SEA_DERIVED_ENERGY ? mul1(0.5f, q) : dv_sqrt_rn(q);
}

// mq_decode_tile's decode with the 8 values left in registers: y[sub][r] is what that function stores at vcol[(sub * 16 + li) * MV_VP + 4 * lg + r].
template <int SP>
__device__ __forceinline__ void mq_decode_regs(const uint4 (&hf)[SP / 32], const char* buf, const float* bias, const int S, const int li, const int lg, float (&y)[2][4]) {
    constexpr int PITCH = SP * 2 + DM_PAD;
    f32x4 acc[2][2];
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
        const float bv = bias[sub * 16 + li];
        acc[sub][0] = f32x4{bv, bv, bv, bv};
        acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ks = 0; ks < SP / 32; ++ks) {
        if (ks * 32 < S) {
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const uint4 wv = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                mma16<__bf16>(hf[ks], wv, acc[sub][ks & 1]);
            }
        }
    }
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int r = 0; r < 4; ++r)   // plain C++: the first reader of an MFMA result must be an instruction the compiler sees
            y[sub][r] = acc[sub][0][r] + acc[sub][1][r];
    }
}

// mq_decode_pair_tile: a wave's 16 members times the tile's 32 columns of derived field X into the value image; bufa, bufb: the LDS images of the two
// sources' tiles; biasa, biasb: their 32 bias entries; vcol: V + the wave's first member.
template <int SP>
__device__ __forceinline__ void mq_decode_pair_tile(const uint4 (&hf)[SP / 32], const char* bufa, const char* bufb, const float* biasa, const float* biasb, const int S,
                                                    const int li, const int lg, const SeaDerivedField& X, float* vcol) {
    float ya[2][4], yb[2][4];
    mq_decode_regs<SP>(hf, bufa, biasa, S, li, lg, ya);
    mq_decode_regs<SP>(hf, bufb, biasb, S, li, lg, yb);
    const int op = X.op;
    const float sa = X.scale_a, ha = X.shift_a, sb = X.scale_b, hb = X.shift_b;
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
        for (int r = 0; r < 4; ++r) vcol[(sub * 16 + li) * MV_VP + 4 * lg + r] = dv_value(op, ya[sub][r], yb[sub][r], sa, ha, sb, hb);
    }
}

template <int SP, int V>
__global__ __launch_bounds__(MV_NT) void decode_derived_quantiles_kernel(const DerivedQuantLaunch L) {
#pragma clang fp reassociate(off)
    constexpr int NW = MV_NW;
    constexpr int NT = MV_NT;
    constexpr int KS = SP / 32;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    constexpr int VP = MV_VP;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images (source a's, source b's); the value image [32][VP]
    float* Vs = reinterpret_cast<float*>(smem + 2 * TILE);
    __shared__ double w_s[VF_MAX_N];
    __shared__ int live_s[VF_MAX_N];
    __shared__ float res_s[DM_TC][QS_MAX_OUT];
    __shared__ float thr_s[SEA_QUANTILE_MAX_LEVELS];

    const SeaDecodeMemberQuantiles& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
    const int S = P.S, C = P.C, Cp = P.Cp, N = P.members, D = L.t.n_derived, nl = P.n_levels, nt = P.n_thr;
    const int bp = blockIdx.x, dg = blockIdx.y, ck = blockIdx.z;   // the derived field and the chunk of its tiles this workgroup reads out
    const int b = bp / P.P, patch = bp - b * P.P;
    const int64_t ld = P.ld;
    const int64_t obase = ((int64_t)bp * D + dg) * ld;

    int lim = C;   // valid columns of this patch: [0, lim) — uniform over the workgroup
    if (P.counts != nullptr) {
        const int cnt = P.counts[patch];
        lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
    }
    const int tpf = (lim + DM_TC - 1) / DM_TC;   // tiles of a field that hold valid columns
    const int tb = ck * MV_CHUNK, te = tpf < tb + MV_CHUNK ? tpf : tb + MV_CHUNK;   // this workgroup's tiles: [tb, te)

    // the weights of the history: a member with w <= 0 or NaN is dead
    int alive = 0;
    if (tid < N) {
        const float wv = P.w != nullptr ? P.w[(int64_t)b * N + tid] : 1.f;
        alive = wv > 0.f ? 1 : 0;   // false for NaN
        w_s[tid] = alive ? (double)wv : 0.0;
        live_s[tid] = alive;
    }
    if (tid < nt) thr_s[tid] = P.thr[(int64_t)tid * D + dg];
    const int n_live = __syncthreads_count(alive);
    const bool empty = n_live == 0;
    if (ck == 0) {   // the columns no tile walks (all of them when the history has no live member or the patch no valid column): 0
        const int c0 = (empty || tpf == 0) ? 0 : tpf * DM_TC;
        for (int64_t c = c0 + tid; c < ld; c += NT) {
            const int64_t at = obase + c;
            for (int k = 0; k < nl; ++k) P.quant[k * P.ld_map + at] = 0.f;
            for (int t = 0; t < nt; ++t) P.exceed[t * P.ld_map + at] = 0.f;
        }
    }
    if (empty || te <= tb) return;   // uniform: nothing to read out in this chunk
    double W = 0.0;
    for (int j = 0; j < N; ++j) W += w_s[j];   // one chain, j ascending; a dead member adds +0

    const int j0 = wave * 16;
    const bool active = j0 < N;                 // uniform over the wave
    const int jm = j0 + li;
    const int64_t m = ((int64_t)b * N + (jm < N ? jm : 0)) * P.P + patch;

    const SeaDerivedField& X = L.t.d[dg];
    const SeaDecodeMseGroup& G = L.g[L.t.gsel[dg]];   // the group that holds both sources
    const int ja = X.a - G.field0, jb = X.b - G.field0;   // the sources inside their group
    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    uint4 hf[KS];
    mq_load_row<SP>(hf, H + m * G.ldh, S, lg);
    const int n_tiles = te - tb, t0a = ja * tpf + tb, t0b = jb * tpf + tb;   // this chunk's tiles among the group's, per source
    uint4 wa[NCH], wb[NCH];
    dm_load_tile<SP, NT>(wa, W2, G.ldw, S, Cp, tpf, t0a, tid);
    dm_load_tile<SP, NT>(wb, W2, G.ldw, S, Cp, tpf, t0b, tid);
    dm_store_tile<SP, NT>(wa, smem, tid);
    dm_store_tile<SP, NT>(wb, smem + TILE, tid);
    __syncthreads();

    for (int t = 0; t < n_tiles; ++t) {
        const int cb = (tb + t) * DM_TC;

        // a: decode both sources, form the derived value, into the value image
        if (active) mq_decode_pair_tile<SP>(hf, smem, smem + TILE, G.bias + ja * Cp + cb, G.bias + jb * Cp + cb, S, li, lg, X, Vs + j0);
        __syncthreads();
        if (t + 1 < n_tiles) {   // in flight behind b
            dm_load_tile<SP, NT>(wa, W2, G.ldw, S, Cp, tpf, t0a + t + 1, tid);
            dm_load_tile<SP, NT>(wb, W2, G.ldw, S, Cp, tpf, t0b + t + 1, tid);
        }

        // b: a column per wave at a time
        for (int cl = wave; cl < DM_TC; cl += NW) {
            if (cb + cl >= lim) continue;   // the same word in every lane: a dead column, stage c writes its zeros
            qs_column_wave<V>(Vs + cl * VP, w_s, live_s, N, lane, W, P.level, nl, thr_s, nt, res_s[cl]);
        }
        __syncthreads();

        // c: thread k stores column k of every map
        if (tid < DM_TC) {
            const int c = cb + tid;
            if (c < ld) {
                const int64_t at = obase + c;
                const bool on = c < lim;
                for (int k = 0; k < nl; ++k) P.quant[k * P.ld_map + at] = on ? res_s[tid][k] : 0.f;
                for (int q = 0; q < nt; ++q) P.exceed[q * P.ld_map + at] = on ? res_s[tid][nl + q] : 0.f;
            }
        }
        if (t + 1 < n_tiles) {
            dm_store_tile<SP, NT>(wa, smem, tid);
            dm_store_tile<SP, NT>(wb, smem + TILE, tid);
        }
        __syncthreads();
    }
}

template <int SP, int V>
__global__ __launch_bounds__(MV_NT) void decode_derived_brier_kernel(const DerivedBrierLaunch L) {
#pragma clang fp reassociate(off)
    constexpr int NW = MV_NW;
    constexpr int NT = MV_NT;
    constexpr int KS = SP / 32;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    constexpr int VP = MV_VP;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    static_assert(DM_TC * BS_MAX_T <= NT, "a thread per (column, threshold)");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images (source a's, source b's); the value image [32][VP]
    float* Vs = reinterpret_cast<float*>(smem + 2 * TILE);
    __shared__ double lw_s[VF_MAX_N], w_s[VF_MAX_N];
    __shared__ int live_s[VF_MAX_N];
    __shared__ BsCell cell_s[DM_TC];
    __shared__ double term_s[BS_MAX_T * BS_SUMS][DM_TC];
    __shared__ int hist_s[2 * BS_MAX_T * (VF_MAX_N + 1)];   // [hist | hits][t][m] at the call's T and N
    __shared__ float y_s[DM_TC], pv_s[DM_TC], thr_s[BS_MAX_T];

    const SeaDecodeMemberBrier& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
    const int S = P.S, C = P.C, Cp = P.Cp, N = P.members, D = L.t.n_derived, T = P.n_thr, words = L.words;
    const int bp = blockIdx.x, dg = blockIdx.y, ck = blockIdx.z, Q = gridDim.z;
    const int b = bp / P.P, patch = bp - b * P.P;
    const int64_t ld = P.ld_out;
    const int64_t obase = ((int64_t)bp * D + dg) * ld;
    const int nb = T * (N + 1);
    double* const wsum = reinterpret_cast<double*>(P.work) + (((int64_t)bp * Q + ck) * D + dg) * words;
    int32_t* const whist = reinterpret_cast<int32_t*>(wsum + T * BS_SUMS);

    int lim = C;   // valid columns of this patch: [0, lim) — uniform over the workgroup
    if (P.counts != nullptr) {
        const int cnt = P.counts[patch];
        lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
    }
    const int tpf = (lim + DM_TC - 1) / DM_TC;   // tiles of a field that hold valid columns
    const int tb = ck * MV_CHUNK, te = tpf < tb + MV_CHUNK ? tpf : tb + MV_CHUNK;   // this workgroup's tiles: [tb, te)

    for (int r = tid; r < 2 * nb; r += NT) hist_s[r] = 0;
    if (tid < T) thr_s[tid] = P.thr[(int64_t)tid * D + dg];
    double W;
    const int n_live = bs_history_weights(P.logw, b, N, tid, lw_s, w_s, live_s, W);   // two barriers: hist_s and thr_s are set behind them
    const bool unscored = n_live < 0;
    if (patch == 0 && dg == 0 && ck == 0 && tid == 0) P.status[b] = n_live;
    if (ck == 0 && (P.prob != nullptr || P.brier != nullptr)) {   // the columns no tile walks (all of them when the history is not scored or the patch has no valid column): 0
        const int c0 = (unscored || tpf == 0) ? 0 : tpf * DM_TC;
        for (int64_t c = c0 + tid; c < ld; c += NT) {
            const int64_t at = obase + c;
            for (int t = 0; t < T; ++t) {
                if (P.prob != nullptr) P.prob[t * P.ld_map + at] = 0.f;
                if (P.brier != nullptr) P.brier[t * P.ld_map + at] = 0.f;
            }
        }
    }
    if (unscored || te <= tb) {   // uniform: nothing to score in this chunk
        for (int e = tid; e < words; e += NT) wsum[e] = 0.0;   // the sums, and the int32 bins: all bits zero
        return;
    }

    const int j0 = wave * 16;
    const bool active = j0 < N;                 // uniform over the wave
    const int jm = j0 + li;
    const int64_t m = ((int64_t)b * N + (jm < N ? jm : 0)) * P.P + patch;
    double acc_sum = 0.0;                       // threads 0 .. 5 T - 1: the derived field's running sums

    const SeaDerivedField& X = L.t.d[dg];
    const SeaDecodeMseGroup& G = L.g[L.t.gsel[dg]];   // the group that holds both sources
    const int ja = X.a - G.field0, jb = X.b - G.field0;   // the sources inside their group
    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    uint4 hf[KS];
    mq_load_row<SP>(hf, H + m * G.ldh, S, lg);
    const int n_tiles = te - tb, t0a = ja * tpf + tb, t0b = jb * tpf + tb;   // this chunk's tiles among the group's, per source
    uint4 wa[NCH], wb[NCH];
    dm_load_tile<SP, NT>(wa, W2, G.ldw, S, Cp, tpf, t0a, tid);
    dm_load_tile<SP, NT>(wb, W2, G.ldw, S, Cp, tpf, t0b, tid);
    dm_store_tile<SP, NT>(wa, smem, tid);
    dm_store_tile<SP, NT>(wb, smem + TILE, tid);
    __syncthreads();

    for (int t = 0; t < n_tiles; ++t) {
        const int cb = (tb + t) * DM_TC;

        // a: the columns' weights and readings (decode_member_brier_kernel's, by derived field); decode both sources into the value image
        if (tid < DM_TC) {
            const int c = cb + tid;
            float w = 0.f;
            if (c < lim) {
                const float pf = P.prec_field != nullptr ? P.prec_field[dg] : 1.f;
                const float pm = P.prec != nullptr ? P.prec[(int64_t)bp * P.ld_prow + (int64_t)dg * P.ld_pfield + c] : 1.f;
                w = mul1(pf > 0.f ? pf : 0.f, pm > 0.f ? pm : 0.f);
            }
            const bool on = w > 0.f;   // false for NaN
            pv_s[tid] = on ? w : 0.f;
            y_s[tid] = on ? P.obs[(int64_t)bp * P.ld_row + (int64_t)dg * P.ld_field + c] : 0.f;
        }
        if (active) mq_decode_pair_tile<SP>(hf, smem, smem + TILE, G.bias + ja * Cp + cb, G.bias + jb * Cp + cb, S, li, lg, X, Vs + j0);
        __syncthreads();
        if (t + 1 < n_tiles) {   // in flight behind b
            dm_load_tile<SP, NT>(wa, W2, G.ldw, S, Cp, tpf, t0a + t + 1, tid);
            dm_load_tile<SP, NT>(wb, W2, G.ldw, S, Cp, tpf, t0b + t + 1, tid);
        }

        // b: a column per wave at a time
        for (int cl = wave; cl < DM_TC; cl += NW) {
            const float pv = pv_s[cl];
            if (!(pv > 0.f)) {   // the same word in every lane
                if (lane == 0) cell_s[cl].state = 1;
                continue;
            }
            bs_column_wave<V>(Vs + cl * VP, w_s, live_s, N, lane, W, y_s[cl], pv, thr_s, T, &cell_s[cl]);
        }
        __syncthreads();

        // c: thread (k, q) finishes threshold q of column k
        if (tid < DM_TC * T) {
            const int k = tid & (DM_TC - 1), q = tid / DM_TC;
            double tm[BS_SUMS];
            const BsOut o = bs_finish_cell(cell_s[k], q, y_s[k], thr_s[q], tm);
            if (o.m >= 0) {   // LDS, integers: the order does not matter; 0 <= m <= N
                atomicAdd(&hist_s[q * (N + 1) + o.m], 1);
                if (o.o) atomicAdd(&hist_s[nb + q * (N + 1) + o.m], 1);
            }
            const int c = cb + k;
            if (c < ld) {
                const int64_t at = q * P.ld_map + obase + c;
                if (P.prob != nullptr) P.prob[at] = o.prob;
                if (P.brier != nullptr) P.brier[at] = o.brier;
            }
#pragma unroll
            for (int i = 0; i < BS_SUMS; ++i) term_s[q * BS_SUMS + i][k] = tm[i];
        }
        if (t + 1 < n_tiles) {
            dm_store_tile<SP, NT>(wa, smem, tid);
            dm_store_tile<SP, NT>(wb, smem + TILE, tid);
        }
        __syncthreads();

        // d: the derived field's sums, columns ascending (the next tile's terms are filed two barriers ahead)
        if (tid < T * BS_SUMS)
            for (int k = 0; k < DM_TC; ++k) acc_sum += term_s[tid][k];
    }
    if (tid < T * BS_SUMS) wsum[tid] = acc_sum;
    for (int r = tid; r < 2 * nb; r += NT) whist[r] = hist_s[r];   // every integer add lies behind the last tile's barrier
}

template <int SP, int V>
static void derived_quantiles_launch(const DerivedQuantLaunch& L, dim3 grid, hipStream_t s) {
    constexpr int lds = mv_lds_bytes<SP>();
    static bool set_on[64] = {false};   // per device: the dynamic part is 100 kB at SP = 640, above the 64 kB a kernel gets without the attribute
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_derived_quantiles_kernel<SP, V>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_derived_quantiles_kernel<SP, V><<<grid, dim3(MV_NT), lds, s>>>(L);
    sea_note_form("decode.derived_quantiles", SP, lds);
}

template <int V>
static void derived_quantiles_dispatch(const DerivedQuantLaunch& L, dim3 grid, hipStream_t s) {
    if (L.p.S <= 128) derived_quantiles_launch<128, V>(L, grid, s);
    else if (L.p.S <= 256) derived_quantiles_launch<256, V>(L, grid, s);
    else if (L.p.S <= 384) derived_quantiles_launch<384, V>(L, grid, s);
    else if (L.p.S <= 512) derived_quantiles_launch<512, V>(L, grid, s);
    else derived_quantiles_launch<640, V>(L, grid, s);
}

template <int SP, int V>
static void derived_brier_launch(const DerivedBrierLaunch& L, dim3 grid, hipStream_t s) {
    constexpr int lds = mv_lds_bytes<SP>();
    static bool set_on[64] = {false};   // per device, as above
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_derived_brier_kernel<SP, V>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_derived_brier_kernel<SP, V><<<grid, dim3(MV_NT), lds, s>>>(L);
    sea_note_form("decode.derived_brier", SP, lds);
}

template <int V>
static void derived_brier_dispatch(const DerivedBrierLaunch& L, dim3 grid, hipStream_t s) {
    if (L.p.S <= 128) derived_brier_launch<128, V>(L, grid, s);
    else if (L.p.S <= 256) derived_brier_launch<256, V>(L, grid, s);
    else if (L.p.S <= 384) derived_brier_launch<384, V>(L, grid, s);
    else if (L.p.S <= 512) derived_brier_launch<512, V>(L, grid, s);
    else derived_brier_launch<640, V>(L, grid, s);
}

// The checks the two derived entry points share, under the entry point's name `who`: the sizes, the groups (the member entry points' checks) and the
// derived table.  SEA_OK, or SEA_EINVAL with the message set.
static int derived_check(const char* who, const SeaDecodeMseGroup* groups, int n_groups, const SeaDerivedField* derived, int n_derived, int M, int S, int C, int Cp, int Pn,
                         int members, int n_fields_total) {
    SEA_REQUIRE(M >= 1, "%s: M=%d must be positive", who, M);
    SEA_REQUIRE(S >= 8 && S % 8 == 0, "%s: S=%d must be a positive multiple of 8", who, S);
    SEA_REQUIRE(Cp >= 32 && Cp % 32 == 0, "%s: Cp=%d must be a positive multiple of 32", who, Cp);
    SEA_REQUIRE(C >= 1 && C <= Cp, "%s: C=%d must lie in 1..Cp=%d", who, C, Cp);
    SEA_REQUIRE(Pn >= 1, "%s: P=%d must be positive", who, Pn);
    SEA_REQUIRE(members >= 1, "%s: members=%d must be positive", who, members);
    SEA_REQUIRE((int64_t)M % ((int64_t)Pn * members) == 0, "%s: M=%d is not a multiple of P * members = %d * %d", who, M, Pn, members);
    SEA_REQUIRE(n_fields_total >= 1 && n_fields_total <= 65535, "%s: n_fields_total=%d outside 1..65535", who, n_fields_total);
    const int64_t BP = (int64_t)M / members, B = BP / Pn;
    SEA_REQUIRE(BP <= 0x7fffffffLL && B <= 65535, "%s: %lld histories; a launch carries up to 65535", who, (long long)B);
    int64_t covered = 0;
    for (int g = 0; g < n_groups; ++g) {
        const SeaDecodeMseGroup& G = groups[g];
        SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr, "%s: group %d: null pointer", who, g);
        SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias), "%s: group %d: pointers must be 16-byte aligned", who, g);
        SEA_REQUIRE(G.ldh >= S && G.ldh % 8 == 0 && G.ldw >= S && G.ldw % 8 == 0, "%s: group %d: row strides ldh=%d ldw=%d must cover S=%d and be multiples of 8", who, g,
                    G.ldh, G.ldw, S);
        SEA_REQUIRE(G.n_fields >= 1 && G.field0 >= 0 && (int64_t)G.field0 + G.n_fields <= n_fields_total, "%s: group %d: n_fields=%d, field0=%d outside the %d fields", who, g,
                    G.n_fields, G.field0, n_fields_total);
        SEA_REQUIRE((int64_t)G.n_fields * Cp <= 0x7fffffffLL / 2, "%s: group %d: too many output columns", who, g);
        for (int h = 0; h < g; ++h)
            SEA_REQUIRE(G.field0 >= groups[h].field0 + groups[h].n_fields || groups[h].field0 >= G.field0 + G.n_fields,
                        "%s: group %d: its fields overlap those of group %d (a cell is decoded once)", who, g, h);
        covered += G.n_fields;
    }
    SEA_REQUIRE(covered == n_fields_total, "%s: the groups cover %lld of the %d fields (every field needs exactly one group)", who, (long long)covered, n_fields_total);
    for (int i = 0; i < n_derived; ++i) {
        const SeaDerivedField& X = derived[i];
        SEA_REQUIRE(X.op == SEA_DERIVED_MAGNITUDE || X.op == SEA_DERIVED_ENERGY || X.op == SEA_DERIVED_DIFFERENCE,
                    "%s: derived field %d: unknown op %d (SEA_DERIVED_MAGNITUDE, SEA_DERIVED_ENERGY or SEA_DERIVED_DIFFERENCE)", who, i, X.op);
        SEA_REQUIRE(X.a >= 0 && X.a < n_fields_total && X.b >= 0 && X.b < n_fields_total, "%s: derived field %d: sources a=%d, b=%d outside the %d fields", who, i, X.a, X.b,
                    n_fields_total);
        SEA_REQUIRE(X.a != X.b, "%s: derived field %d: a == b = %d (two different source fields are needed)", who, i, X.a);
        SEA_REQUIRE(std::isfinite(X.scale_a) && std::isfinite(X.shift_a) && std::isfinite(X.scale_b) && std::isfinite(X.shift_b),
                    "%s: derived field %d: a coefficient is not finite (scale_a=%g shift_a=%g scale_b=%g shift_b=%g)", who, i, (double)X.scale_a, (double)X.shift_a,
                    (double)X.scale_b, (double)X.shift_b);
    }
    return SEA_OK;
}

// What the fused launches do not carry (the caller composes): SEA_OK with the table filled, or SEA_EUNSUPPORTED with the message set.
static int derived_resolve(const char* who, const SeaDecodeMseGroup* groups, int n_groups, const SeaDerivedField* derived, int n_derived, int S, int members, DerivedTable& t) {
    if (S > 640) {
        sea_set_error("%s: unsupported: hidden width S=%d above 640", who, S);
        return SEA_EUNSUPPORTED;
    }
    if (members > VF_MAX_N) {
        sea_set_error("%s: unsupported: members=%d above %d", who, members, VF_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    memset(&t, 0, sizeof(t));
    t.n_derived = n_derived;
    for (int i = 0; i < n_derived; ++i) {
        int ga = -1, gb = -1;
        for (int g = 0; g < n_groups; ++g) {
            if (derived[i].a >= groups[g].field0 && derived[i].a < groups[g].field0 + groups[g].n_fields) ga = g;
            if (derived[i].b >= groups[g].field0 && derived[i].b < groups[g].field0 + groups[g].n_fields) gb = g;
        }
        if (ga != gb) {
            sea_set_error("%s: unsupported: derived field %d: its sources a=%d and b=%d lie in different groups (%d and %d)", who, i, derived[i].a, derived[i].b, ga, gb);
            return SEA_EUNSUPPORTED;
        }
        t.d[i] = derived[i];
        t.gsel[i] = ga;
    }
    return SEA_OK;
}

extern "C" int sea_decode_derived_quantiles(const SeaDecodeMseGroup* groups, int n_groups, const SeaDerivedField* derived, int n_derived,
                                            const SeaDecodeMemberQuantiles* p, int dtype, void* stream) {
    const char* who = "sea_decode_derived_quantiles";
    SEA_REQUIRE(groups != nullptr && derived != nullptr && p != nullptr, "%s: null argument table", who);
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "%s: n_groups=%d outside 1..%d", who, n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(n_derived >= 1 && n_derived <= SEA_DERIVED_MAX, "%s: n_derived=%d outside 1..%d", who, n_derived, SEA_DERIVED_MAX);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "%s: bad dtype %d", who, dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("%s: unsupported: bf16 only (the fp32 decoder composes the decode, the derived values and a sort)", who);
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeMemberQuantiles& P = *p;
    SEA_REQUIRE(P.n_levels >= 0 && P.n_levels <= SEA_QUANTILE_MAX_LEVELS && P.n_thr >= 0 && P.n_thr <= SEA_QUANTILE_MAX_LEVELS && P.n_levels + P.n_thr >= 1,
                "%s: n_levels=%d and n_thr=%d must lie in 0..%d and not both be 0", who, P.n_levels, P.n_thr, SEA_QUANTILE_MAX_LEVELS);
    for (int k = 0; k < P.n_levels; ++k)
        SEA_REQUIRE(P.level[k] >= 0.f && P.level[k] <= 1.f, "%s: level[%d]=%g must be finite and lie in [0, 1]", who, k, (double)P.level[k]);
    SEA_REQUIRE((P.n_levels == 0 || P.quant != nullptr) && (P.n_thr == 0 || (P.thr != nullptr && P.exceed != nullptr)),
                "%s: null pointer (quant is required with levels, thr and exceed with thresholds; w and counts may be NULL)", who);
    const int rc = derived_check(who, groups, n_groups, derived, n_derived, P.M, P.S, P.C, P.Cp, P.P, P.members, P.n_fields_total);
    if (rc != SEA_OK) return rc;
    const int64_t BP = (int64_t)P.M / P.members;   // (history, patch) pairs
    SEA_REQUIRE(P.ld >= P.C && P.ld <= 0x7fffffffLL && P.ld_map >= BP * n_derived * P.ld, "%s: ld=%lld must cover C=%d, and ld_map=%lld a whole map of %lld floats", who,
                (long long)P.ld, P.C, (long long)P.ld_map, (long long)(BP * n_derived * P.ld));
    SEA_REQUIRE(sea_aligned4(P.w) && sea_aligned4(P.counts) && sea_aligned4(P.thr) && sea_aligned4(P.quant) && sea_aligned4(P.exceed),
                "%s: misaligned pointer (f32 and int32 buffers need 4 bytes)", who);
    SEA_REQUIRE(mv_chunks(P.Cp) <= 65535, "%s: Cp=%d has too many column chunks", who, P.Cp);

    DerivedQuantLaunch L;
    memset(&L, 0, sizeof(L));
    const int ru = derived_resolve(who, groups, n_groups, derived, n_derived, P.S, P.members, L.t);
    if (ru != SEA_OK) return ru;
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)BP, (unsigned)n_derived, (unsigned)mv_chunks(P.Cp));
    if (P.members <= 64) derived_quantiles_dispatch<1>(L, grid, s);
    else derived_quantiles_dispatch<2>(L, grid, s);
    SEA_CHECK_LAUNCH("sea_decode_derived_quantiles");
    return SEA_OK;
}

extern "C" int sea_decode_derived_brier(const SeaDecodeMseGroup* groups, int n_groups, const SeaDerivedField* derived, int n_derived, const SeaDecodeMemberBrier* p,
                                        int dtype, void* stream) {
    const char* who = "sea_decode_derived_brier";
    SEA_REQUIRE(groups != nullptr && derived != nullptr && p != nullptr, "%s: null argument table", who);
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "%s: n_groups=%d outside 1..%d", who, n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(n_derived >= 1 && n_derived <= SEA_DERIVED_MAX, "%s: n_derived=%d outside 1..%d", who, n_derived, SEA_DERIVED_MAX);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "%s: bad dtype %d", who, dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("%s: unsupported: bf16 only (the fp32 decoder composes the decode, the derived values and the formulas)", who);
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeMemberBrier& P = *p;
    SEA_REQUIRE(P.obs != nullptr && P.thr != nullptr && P.sums != nullptr && P.hist != nullptr && P.hits != nullptr && P.status != nullptr && P.work != nullptr,
                "%s: null pointer (obs, thr, sums, hist, hits, status and work are required; prec_field, prec, counts, logw and the maps may be NULL)", who);
    SEA_REQUIRE(P.n_thr >= 1 && P.n_thr <= BS_MAX_T, "%s: n_thr=%d outside 1..%d", who, P.n_thr, BS_MAX_T);
    const int rc = derived_check(who, groups, n_groups, derived, n_derived, P.M, P.S, P.C, P.Cp, P.P, P.members, P.n_fields_total);
    if (rc != SEA_OK) return rc;
    SEA_REQUIRE(P.ld_field >= P.C && P.ld_row >= 0, "%s: obs strides ld_row=%lld, ld_field=%lld must cover C=%d", who, (long long)P.ld_row, (long long)P.ld_field, P.C);
    SEA_REQUIRE(P.prec == nullptr || (P.ld_pfield >= P.C && P.ld_prow >= 0), "%s: prec strides ld_prow=%lld, ld_pfield=%lld must cover C=%d", who, (long long)P.ld_prow,
                (long long)P.ld_pfield, P.C);
    const int64_t BP = (int64_t)P.M / P.members;   // (history, patch) pairs
    const int64_t B = BP / P.P;
    SEA_REQUIRE((P.prob == nullptr && P.brier == nullptr) || (P.ld_out >= P.C && P.ld_out <= 0x7fffffffLL && P.ld_map >= BP * n_derived * P.ld_out),
                "%s: ld_out=%lld must cover C=%d, and ld_map=%lld a whole map", who, (long long)P.ld_out, P.C, (long long)P.ld_map);
    SEA_REQUIRE(P.accumulate == 0 || P.accumulate == 1, "%s: accumulate=%d must be 0 or 1", who, P.accumulate);
    SEA_REQUIRE(sea_aligned4(P.obs) && sea_aligned4(P.prec_field) && sea_aligned4(P.prec) && sea_aligned4(P.counts) && sea_aligned4(P.logw) && sea_aligned4(P.thr) &&
                    sea_aligned4(P.prob) && sea_aligned4(P.brier) && sea_aligned4(P.status) && (reinterpret_cast<uintptr_t>(P.sums) & 7u) == 0 &&
                    (reinterpret_cast<uintptr_t>(P.hist) & 7u) == 0 && (reinterpret_cast<uintptr_t>(P.hits) & 7u) == 0 && (reinterpret_cast<uintptr_t>(P.work) & 7u) == 0,
                "%s: misaligned pointer (f32 and int32 buffers need 4 bytes; sums, hist, hits and work 8)", who);

    DerivedBrierLaunch L;
    memset(&L, 0, sizeof(L));
    const int ru = derived_resolve(who, groups, n_groups, derived, n_derived, P.S, P.members, L.t);
    if (ru != SEA_OK) return ru;
    const int64_t need = sea_decode_member_brier_ws_bytes((int)B, P.P, n_derived, P.members, P.Cp, P.n_thr);
    SEA_REQUIRE(P.work_bytes >= need, "%s: work_bytes=%lld below the %lld that sea_decode_member_brier_ws_bytes(B=%d, P=%d, n_derived=%d, members=%d, Cp=%d, n_thr=%d) asks for",
                who, (long long)P.work_bytes, (long long)need, (int)B, P.P, n_derived, P.members, P.Cp, P.n_thr);
    SEA_REQUIRE((int64_t)P.P * mv_chunks(P.Cp) <= 0x7fffffffLL && mv_chunks(P.Cp) <= 65535, "%s: Cp=%d has too many column chunks", who, P.Cp);

    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    L.words = (int)bs_words(P.n_thr, P.members);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)BP, (unsigned)n_derived, (unsigned)mv_chunks(P.Cp));
    if (P.members <= 64) derived_brier_dispatch<1>(L, grid, s);
    else derived_brier_dispatch<2>(L, grid, s);
    SeaDecodeMemberBrier Pd = P;   // the finish launch reads its partials by derived field
    Pd.n_fields_total = n_derived;
    member_brier_finish_kernel<<<dim3((unsigned)B, (unsigned)(n_derived * P.n_thr)), dim3(256), 0, s>>>(Pd, mv_chunks(P.Cp), L.words);
    SEA_CHECK_LAUNCH("sea_decode_derived_brier");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_derived_verify: sea_decode_member_verify for DERIVED fields — per cell the mean, spread, CRPS, PIT and rank of the members' derived
// values, per (history, derived field) the fp64 sums and the rank histogram (include/sea_hip.h states the definitions).  Launch 1 is
// decode_member_verify_kernel with grid.y = n_derived and the decode of its stage a replaced by the two-source decode of the derived kernels above
// (mq_decode_pair_tile; the W2 stream a_0, b_0, a_1, b_1, ... through the two LDS images, two staging sets fetched behind stage b and stored in stage
// c, the hidden rows loaded once).  The preamble and the stages b, c, d are RESTATED from decode_member_verify_kernel line for line, indexed by
// derived field — that kernel stays textually unchanged, and a shared body would have put its pinned bits behind a refactoring; the arithmetic
// itself is shared: vf_score_wave and vf_finish_reading (verify_score.hpp) score a derived cell as they score a cell of the member launch and a
// sensor of sea_ensemble_verify.  Three barriers per tile, LDS at mv_lds_bytes<SP>() plus the member kernel's static part, the member launch's
// workspace layout [(history, patch), chunk, derived field]; member_verify_finish_kernel adds the partials, handed n_derived for F.
struct DerivedVerifyLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeMemberVerify p;
    DerivedTable t;
    int words;   // 8-byte words per (history, patch, chunk, derived field) of the workspace
};

template <int SP, int V>
__global__ __launch_bounds__(MV_NT) void decode_derived_verify_kernel(const DerivedVerifyLaunch L) {
#pragma clang fp reassociate(off)
    constexpr int NW = MV_NW;
    constexpr int NT = MV_NT;
    constexpr int KS = SP / 32;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    constexpr int VP = MV_VP;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images (source a's, source b's); the value image [32][VP]
    float* Vs = reinterpret_cast<float*>(smem + 2 * TILE);
    __shared__ double lw_s[VF_MAX_N], w_s[VF_MAX_N];
    __shared__ int live_s[VF_MAX_N];
    __shared__ VfReading r_s[DM_TC];
    __shared__ double term_s[VF_SUMS][DM_TC];
    __shared__ int hist_s[VF_MAX_N + 1];
    __shared__ float y_s[DM_TC], pv_s[DM_TC];

    const SeaDecodeMemberVerify& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
    const int S = P.S, C = P.C, Cp = P.Cp, N = P.members, D = L.t.n_derived, words = L.words;
    const int bp = blockIdx.x, dg = blockIdx.y, ck = blockIdx.z, Q = gridDim.z;   // the derived field and the chunk of its tiles this workgroup scores
    const int b = bp / P.P, patch = bp - b * P.P;
    const int64_t ld = P.ld_out;
    const int64_t obase = ((int64_t)bp * D + dg) * ld;
    double* const wsum = reinterpret_cast<double*>(P.work) + (((int64_t)bp * Q + ck) * D + dg) * words;
    int32_t* const whist = reinterpret_cast<int32_t*>(wsum + VF_SUMS);

    int lim = C;   // valid columns of this patch: [0, lim) — uniform over the workgroup
    if (P.counts != nullptr) {
        const int cnt = P.counts[patch];
        lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
    }
    const int tpf = (lim + DM_TC - 1) / DM_TC;   // tiles of a field that hold valid columns
    const int tb = ck * MV_CHUNK, te = tpf < tb + MV_CHUNK ? tpf : tb + MV_CHUNK;   // this workgroup's tiles: [tb, te)

    // the weights of the history (decode_member_verify_kernel's, line for line)
    int invalid = 0, alive = 0;
    if (tid < N) {
        const float lw = P.logw != nullptr ? P.logw[(int64_t)b * N + tid] : 0.f;
        invalid = (lw != lw || lw == INFINITY) ? 1 : 0;
        alive = (!invalid && lw != -INFINITY) ? 1 : 0;
        lw_s[tid] = (double)lw;
        live_s[tid] = alive;
    }
    for (int r = tid; r <= N; r += NT) hist_s[r] = 0;
    const int n_live = __syncthreads_count(alive);
    invalid = __syncthreads_or(invalid);
    const bool unscored = invalid || n_live == 0;
    if (patch == 0 && dg == 0 && ck == 0 && tid == 0) P.status[b] = unscored ? -1 : n_live;
    if (ck == 0) {   // the columns no tile walks (all of them when the history is not scored or the patch has no valid column): dead
        const int c0 = (unscored || tpf == 0) ? 0 : tpf * DM_TC;
        for (int64_t c = c0 + tid; c < ld; c += NT) {
            const int64_t at = obase + c;
            if (P.mean != nullptr) P.mean[at] = 0.f;
            if (P.spread != nullptr) P.spread[at] = 0.f;
            if (P.crps != nullptr) P.crps[at] = 0.f;
            if (P.pit != nullptr) P.pit[at] = 0.f;
            if (P.rank != nullptr) P.rank[at] = -1;
        }
    }
    if (unscored || te <= tb) {   // uniform: nothing to score in this chunk
        for (int e = tid; e < words; e += NT) wsum[e] = 0.0;   // the sums, and the int32 bins: all bits zero
        return;
    }
    double mx = -INFINITY;
    for (int j = 0; j < N; ++j) mx = lw_s[j] > mx ? lw_s[j] : mx;
    if (tid < N) w_s[tid] = alive ? exp(lw_s[tid] - mx) : 0.0;
    __syncthreads();
    double W = 0.0;
    for (int j = 0; j < N; ++j) W += w_s[j];
    const double my_w = tid < N ? w_s[tid] / W : 0.0;
    __syncthreads();   // every thread has read the exponentials
    if (tid < N) w_s[tid] = my_w;
    __syncthreads();
    double q = 0.0;
    for (int j = 0; j < N; ++j) q = fma(w_s[j], w_s[j], q);
    const double cq = P.unbiased ? 1.0 - q : 1.0;

    const int j0 = wave * 16;
    const bool active = j0 < N;                 // uniform over the wave
    const int jm = j0 + li;
    const int64_t m = ((int64_t)b * N + (jm < N ? jm : 0)) * P.P + patch;
    double acc_sum = 0.0;                       // threads 0 .. 7: the derived field's running sums

    const SeaDerivedField& X = L.t.d[dg];
    const SeaDecodeMseGroup& G = L.g[L.t.gsel[dg]];   // the group that holds both sources
    const int ja = X.a - G.field0, jb = X.b - G.field0;   // the sources inside their group
    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    uint4 hf[KS];
    mq_load_row<SP>(hf, H + m * G.ldh, S, lg);
    const int n_tiles = te - tb, t0a = ja * tpf + tb, t0b = jb * tpf + tb;   // this chunk's tiles among the group's, per source
    uint4 wa[NCH], wb[NCH];
    dm_load_tile<SP, NT>(wa, W2, G.ldw, S, Cp, tpf, t0a, tid);
    dm_load_tile<SP, NT>(wb, W2, G.ldw, S, Cp, tpf, t0b, tid);
    dm_store_tile<SP, NT>(wa, smem, tid);
    dm_store_tile<SP, NT>(wb, smem + TILE, tid);
    __syncthreads();

    for (int t = 0; t < n_tiles; ++t) {
        const int cb = (tb + t) * DM_TC;

        // a: the columns' weights and readings (decode_member_verify_kernel's, by derived field); decode both sources into the value image
        if (tid < DM_TC) {
            const int c = cb + tid;
            float w = 0.f;
            if (c < lim) {
                const float pf = P.prec_field != nullptr ? P.prec_field[dg] : 1.f;
                const float pm = P.prec != nullptr ? P.prec[(int64_t)bp * P.ld_prow + (int64_t)dg * P.ld_pfield + c] : 1.f;
                w = mul1(pf > 0.f ? pf : 0.f, pm > 0.f ? pm : 0.f);
            }
            const bool on = w > 0.f;   // false for NaN
            pv_s[tid] = on ? w : 0.f;
            y_s[tid] = on ? P.obs[(int64_t)bp * P.ld_row + (int64_t)dg * P.ld_field + c] : 0.f;
        }
        if (active) mq_decode_pair_tile<SP>(hf, smem, smem + TILE, G.bias + ja * Cp + cb, G.bias + jb * Cp + cb, S, li, lg, X, Vs + j0);
        __syncthreads();
        if (t + 1 < n_tiles) {   // in flight behind b
            dm_load_tile<SP, NT>(wa, W2, G.ldw, S, Cp, tpf, t0a + t + 1, tid);
            dm_load_tile<SP, NT>(wb, W2, G.ldw, S, Cp, tpf, t0b + t + 1, tid);
        }

        // b: a column per wave at a time
        for (int cl = wave; cl < DM_TC; cl += NW) {
            const float pv = pv_s[cl];
            if (!(pv > 0.f)) {   // the same word in every lane
                if (lane == 0) r_s[cl].state = 1;
                continue;
            }
            const VfReading r = vf_score_wave<V>(Vs + cl * VP, w_s, live_s, N, lane, y_s[cl], pv);
            if (lane == 0) r_s[cl] = r;
        }
        __syncthreads();

        // c: thread k finishes column k
        if (tid < DM_TC) {
            double tm[VF_SUMS];
            const VfReading r = r_s[tid];
            const VfOut o = vf_finish_reading(r, y_s[tid], pv_s[tid], cq, tm);
            if (r.state == 0) atomicAdd(&hist_s[o.rank], 1);   // LDS, integers: the order does not matter; 0 <= rank <= N
            const int c = cb + tid;
            if (c < ld) {
                const int64_t at = obase + c;
                if (P.mean != nullptr) P.mean[at] = o.mean;
                if (P.spread != nullptr) P.spread[at] = o.spread;
                if (P.crps != nullptr) P.crps[at] = o.crps;
                if (P.pit != nullptr) P.pit[at] = o.pit;
                if (P.rank != nullptr) P.rank[at] = o.rank;
            }
#pragma unroll
            for (int i = 0; i < VF_SUMS; ++i) term_s[i][tid] = tm[i];
        }
        if (t + 1 < n_tiles) {
            dm_store_tile<SP, NT>(wa, smem, tid);
            dm_store_tile<SP, NT>(wb, smem + TILE, tid);
        }
        __syncthreads();

        // d: the derived field's sums, columns ascending (the next tile's terms are filed two barriers ahead)
        if (tid < VF_SUMS)
            for (int k = 0; k < DM_TC; ++k) acc_sum += term_s[tid][k];
    }
    if (tid < VF_SUMS) wsum[tid] = acc_sum;
    for (int r = tid; r <= N; r += NT) whist[r] = hist_s[r];   // every integer add lies behind the last tile's barrier
}

template <int SP, int V>
static void derived_verify_launch(const DerivedVerifyLaunch& L, dim3 grid, hipStream_t s) {
    constexpr int lds = mv_lds_bytes<SP>();
    static bool set_on[64] = {false};   // per device, as above
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_derived_verify_kernel<SP, V>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_derived_verify_kernel<SP, V><<<grid, dim3(MV_NT), lds, s>>>(L);
    sea_note_form("decode.derived_verify", SP, lds);
}

template <int V>
static void derived_verify_dispatch(const DerivedVerifyLaunch& L, dim3 grid, hipStream_t s) {
    if (L.p.S <= 128) derived_verify_launch<128, V>(L, grid, s);
    else if (L.p.S <= 256) derived_verify_launch<256, V>(L, grid, s);
    else if (L.p.S <= 384) derived_verify_launch<384, V>(L, grid, s);
    else if (L.p.S <= 512) derived_verify_launch<512, V>(L, grid, s);
    else derived_verify_launch<640, V>(L, grid, s);
}

extern "C" int sea_decode_derived_verify(const SeaDecodeMseGroup* groups, int n_groups, const SeaDerivedField* derived, int n_derived, const SeaDecodeMemberVerify* p,
                                         int dtype, void* stream) {
    const char* who = "sea_decode_derived_verify";
    SEA_REQUIRE(groups != nullptr && derived != nullptr && p != nullptr, "%s: null argument table", who);
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "%s: n_groups=%d outside 1..%d", who, n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(n_derived >= 1 && n_derived <= SEA_DERIVED_MAX, "%s: n_derived=%d outside 1..%d", who, n_derived, SEA_DERIVED_MAX);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "%s: bad dtype %d", who, dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("%s: unsupported: bf16 only (the fp32 decoder composes the decode, the derived values and sea_ensemble_verify's formulas)", who);
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeMemberVerify& P = *p;
    SEA_REQUIRE(P.obs != nullptr && P.sums != nullptr && P.hist != nullptr && P.status != nullptr && P.work != nullptr,
                "%s: null pointer (obs, sums, hist, status and work are required; prec_field, prec, counts, logw and the maps may be NULL)", who);
    const int rc = derived_check(who, groups, n_groups, derived, n_derived, P.M, P.S, P.C, P.Cp, P.P, P.members, P.n_fields_total);
    if (rc != SEA_OK) return rc;
    SEA_REQUIRE(P.ld_field >= P.C && P.ld_row >= 0, "%s: obs strides ld_row=%lld, ld_field=%lld must cover C=%d", who, (long long)P.ld_row, (long long)P.ld_field, P.C);
    SEA_REQUIRE(P.prec == nullptr || (P.ld_pfield >= P.C && P.ld_prow >= 0), "%s: prec strides ld_prow=%lld, ld_pfield=%lld must cover C=%d", who, (long long)P.ld_prow,
                (long long)P.ld_pfield, P.C);
    SEA_REQUIRE((P.mean == nullptr && P.spread == nullptr && P.crps == nullptr && P.pit == nullptr && P.rank == nullptr) || (P.ld_out >= P.C && P.ld_out <= 0x7fffffffLL),
                "%s: ld_out=%lld must cover C=%d", who, (long long)P.ld_out, P.C);
    SEA_REQUIRE((P.unbiased == 0 || P.unbiased == 1) && (P.accumulate == 0 || P.accumulate == 1), "%s: unbiased=%d and accumulate=%d must be 0 or 1", who, P.unbiased,
                P.accumulate);
    SEA_REQUIRE(sea_aligned4(P.obs) && sea_aligned4(P.prec_field) && sea_aligned4(P.prec) && sea_aligned4(P.counts) && sea_aligned4(P.logw) && sea_aligned4(P.mean) &&
                    sea_aligned4(P.spread) && sea_aligned4(P.crps) && sea_aligned4(P.pit) && sea_aligned4(P.rank) && sea_aligned4(P.status) &&
                    (reinterpret_cast<uintptr_t>(P.sums) & 7u) == 0 && (reinterpret_cast<uintptr_t>(P.hist) & 7u) == 0 && (reinterpret_cast<uintptr_t>(P.work) & 7u) == 0,
                "%s: misaligned pointer (f32 and int32 buffers need 4 bytes; sums, hist and work 8)", who);

    DerivedVerifyLaunch L;
    memset(&L, 0, sizeof(L));
    const int ru = derived_resolve(who, groups, n_groups, derived, n_derived, P.S, P.members, L.t);
    if (ru != SEA_OK) return ru;
    const int64_t BP = (int64_t)P.M / P.members;   // (history, patch) pairs
    const int64_t B = BP / P.P;
    const int64_t need = sea_decode_member_verify_ws_bytes((int)B, P.P, n_derived, P.members, P.Cp);
    SEA_REQUIRE(P.work_bytes >= need, "%s: work_bytes=%lld below the %lld that sea_decode_member_verify_ws_bytes(B=%d, P=%d, n_derived=%d, members=%d, Cp=%d) asks for", who,
                (long long)P.work_bytes, (long long)need, (int)B, P.P, n_derived, P.members, P.Cp);
    SEA_REQUIRE((int64_t)P.P * mv_chunks(P.Cp) <= 0x7fffffffLL && mv_chunks(P.Cp) <= 65535, "%s: Cp=%d has too many column chunks", who, P.Cp);

    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    L.words = (int)mv_words(P.members);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)BP, (unsigned)n_derived, (unsigned)mv_chunks(P.Cp));
    if (P.members <= 64) derived_verify_dispatch<1>(L, grid, s);
    else derived_verify_dispatch<2>(L, grid, s);
    SeaDecodeMemberVerify Pd = P;   // the finish launch reads its partials by derived field
    Pd.n_fields_total = n_derived;
    member_verify_finish_kernel<<<dim3((unsigned)B), dim3(256), 0, s>>>(Pd, mv_chunks(P.Cp), L.words);
    SEA_CHECK_LAUNCH("sea_decode_derived_verify");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_member_crps_grad: the CRPS of the decoded fields per (history, field) WITH its gradient to the hidden rows (include/sea_hip.h states
// the formulas) — decode_member_verify_kernel crossed with stage 2 of decode_mse_kernel.  Launch 1 keeps member_verify's grid, a workgroup per
// (history, patch, field, chunk of MV_CHUNK tiles), and its decode, weights, walk and sums line for line (no maps, no histogram): the fp64 sums
// have that launch's bits.  Per tile, between scoring and the next tile:
//   b  the scoring lanes form G = fw w (sign(x - y) - (2 below + w - 1) / c) in fp64 from what vf_score_wave_ex hands back (0 by selects for a
//      dead member, a dead or bad cell), round it to f32 and then to bf16 ONCE — the leading term, LDS image Gs[member][32 columns] — and round what
//      that rounding left (exact in f32) to bf16 too: the trailing term, image Gt, 0 wherever fw G is a bf16 value.  One bf16 term alone errs by up to
//      2^-8 relative, which a row with a single live cell shows undiminished; with both the operand carries 16 bits;
//   c  the wave that decoded the members 16 w .. 16 w + 15 reads its rows of Gs and Gt as A fragments (k-slot (g, j) = column 4 g + j or 16 + 4 g + j - 4)
//      and multiplies them, the leading term first, against the SAME LDS image of the W2 tile, read column-wise (ds_read_b64_tr_b16), into its [16, SP] fp32 slice of dH —
//      decode_mse_kernel's stage 2 and accumulator layout — while thread k finishes column k and the next tile goes to the other image.
// No barrier is added: Gs and Gt are written between the barriers around b and read between those around c.  After the last tile the slice goes to the
// workgroup's private fp32 partial [members, S] in `work`; a workgroup with nothing to score (an unscored history, a chunk without a valid column)
// writes its zero sums only.  Launch 2 (member_crps_finish_kernel): block b < B adds history b's sums in ascending (patch, chunk) order —
// member_verify_finish_kernel's order — and writes loss[b, f] = float(fw[f] * sums[b, f, 1]); block B + m adds the partials of row m per group in
// ascending (field, chunk) order, passing over the workgroups that wrote none by the same uniform tests, applies gelu'(Z) where Z is given, rounds
// once and writes dH: one writer per element, no floating-point atomics, two runs give the same bits, and nothing of a history depends on another.
// NW is the number of waves: 8 as member_verify (2 waves per SIMD: 256 registers each), or 4 where members <= 64 and the dH slice needs the whole file.
struct MemberCrpsLaunch {
    SeaDecodeMseGroup g[SEA_DECODE_MSE_MAX_GROUPS];
    SeaDecodeMemberCrpsGrad p;
    int n_groups;
    int chunks;
};

constexpr int MC_GP = 36;   // bf16 per member row of the G image (32 columns and 8 bytes of pad: a row is 72 bytes, 8-byte aligned)

__host__ __device__ static inline int64_t mc_sum_bytes(int64_t BP, int Q, int F) { return BP * Q * F * VF_SUMS * 8; }

template <int SP>
constexpr int mc_lds_bytes() { return 2 * DM_TC * (SP * 2 + DM_PAD) + DM_TC * MV_VP * 4 + 2 * VF_MAX_N * MC_GP * 2; }

template <int SP, int V, int NW>
__global__ __launch_bounds__(64 * NW) void decode_member_crps_grad_kernel(const MemberCrpsLaunch L) {
#pragma clang fp reassociate(off)
    constexpr int NT = 64 * NW;
    constexpr int KS = SP / 32;
    constexpr int ST = SP / 16;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    constexpr int VP = MV_VP;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    static_assert(16 * NW >= 64 * V || NW == 8, "the waves decode every member");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images; the value image [32][VP]; the two G images [128][MC_GP] (leading and trailing bf16 term)
    float* Vs = reinterpret_cast<float*>(smem + 2 * TILE);
    __bf16* Gs = reinterpret_cast<__bf16*>(smem + 2 * TILE + DM_TC * VP * 4);
    __bf16* Gt = Gs + VF_MAX_N * MC_GP;
    __shared__ double lw_s[VF_MAX_N], w_s[VF_MAX_N];
    __shared__ int live_s[VF_MAX_N];
    __shared__ VfReading r_s[DM_TC];
    __shared__ double term_s[VF_SUMS][DM_TC];
    __shared__ float y_s[DM_TC], pv_s[DM_TC];

    const SeaDecodeMemberCrpsGrad& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
    const int S = P.S, C = P.C, Cp = P.Cp, N = P.members, F = P.n_fields_total;
    const int bp = blockIdx.x, fg = blockIdx.y, ck = blockIdx.z, Q = gridDim.z;
    const int b = bp / P.P, patch = bp - b * P.P;
    const int64_t slot = ((int64_t)bp * Q + ck) * F + fg;   // this workgroup's place in both parts of the workspace
    double* const wsum = reinterpret_cast<double*>(P.work) + slot * VF_SUMS;
    float* const wpart = reinterpret_cast<float*>(static_cast<char*>(P.work) + mc_sum_bytes(gridDim.x, Q, F)) + slot * N * S;

    int lim = C;   // valid columns of this patch: [0, lim) — uniform over the workgroup
    if (P.counts != nullptr) {
        const int cnt = P.counts[patch];
        lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
    }
    const int tpf = (lim + DM_TC - 1) / DM_TC;
    const int tb = ck * MV_CHUNK, te = tpf < tb + MV_CHUNK ? tpf : tb + MV_CHUNK;

    // the weights of the history (decode_member_verify_kernel's, line for line)
    int invalid = 0, alive = 0;
    if (tid < N) {
        const float lw = P.logw != nullptr ? P.logw[(int64_t)b * N + tid] : 0.f;
        invalid = (lw != lw || lw == INFINITY) ? 1 : 0;
        alive = (!invalid && lw != -INFINITY) ? 1 : 0;
        lw_s[tid] = (double)lw;
        live_s[tid] = alive;
    }
    const int n_live = __syncthreads_count(alive);
    invalid = __syncthreads_or(invalid);
    const bool unscored = invalid || n_live == 0;
    if (patch == 0 && fg == 0 && ck == 0 && tid == 0) P.status[b] = unscored ? -1 : n_live;
    if (unscored || te <= tb) {   // uniform: nothing to score in this chunk; the finish launch passes its partial over
        if (tid < VF_SUMS) wsum[tid] = 0.0;
        return;
    }
    double mx = -INFINITY;
    for (int j = 0; j < N; ++j) mx = lw_s[j] > mx ? lw_s[j] : mx;
    if (tid < N) w_s[tid] = alive ? exp(lw_s[tid] - mx) : 0.0;
    __syncthreads();
    double W = 0.0;
    for (int j = 0; j < N; ++j) W += w_s[j];
    const double my_w = tid < N ? w_s[tid] / W : 0.0;
    __syncthreads();
    if (tid < N) w_s[tid] = my_w;
    __syncthreads();
    double q = 0.0;
    for (int j = 0; j < N; ++j) q = fma(w_s[j], w_s[j], q);
    const double cq = P.unbiased ? 1.0 - q : 1.0;
    float fwv = P.field_weight != nullptr ? P.field_weight[fg] : 1.f;
    fwv = fwv > 0.f ? fwv : 0.f;   // false for NaN
    const double fwd = (double)fwv;

    const int j0 = wave * 16;
    const bool active = j0 < N;
    const int jm = j0 + li;
    const int64_t m = ((int64_t)b * N + (jm < N ? jm : 0)) * P.P + patch;
    double acc_sum = 0.0;

    int gsel = 0;
    for (int gi = 1; gi < L.n_groups; ++gi) gsel = (fg >= L.g[gi].field0 && fg < L.g[gi].field0 + L.g[gi].n_fields) ? gi : gsel;
    const SeaDecodeMseGroup& G = L.g[gsel];
    const int j = fg - G.field0;
    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    uint4 hf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int s = ks * 32 + 8 * lg;
        if (ks * 32 + 32 <= S) {
            hf[ks] = *reinterpret_cast<const uint4*>(H + m * G.ldh + s);
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(H + m * G.ldh + (s < S ? s : 0));
            hf[ks] = s < S ? v : make_uint4(0u, 0u, 0u, 0u);
        }
    }
    f32x4 dh[ST];
#pragma unroll
    for (int st = 0; st < ST; ++st) dh[st] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int n_tiles = te - tb, t0 = j * tpf + tb;
    uint4 wr[NCH];
    dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t0, tid);
    dm_store_tile<SP, NT>(wr, smem, tid);
    __syncthreads();

    typedef dm_s16x4 __attribute__((address_space(3))) * lds_p;
    for (int t = 0; t < n_tiles; ++t) {
        const char* buf = smem + (t & 1) * TILE;
        const int cb = (tb + t) * DM_TC;

        // a: the columns' weights and readings; decode into the value image
        if (tid < DM_TC) {
            const int c = cb + tid;
            float w = 0.f;
            if (c < lim) {
                const float pf = P.prec_field != nullptr ? P.prec_field[fg] : 1.f;
                const float pm = P.prec != nullptr ? P.prec[(int64_t)bp * P.ld_prow + (int64_t)fg * P.ld_pfield + c] : 1.f;
                w = mul1(pf > 0.f ? pf : 0.f, pm > 0.f ? pm : 0.f);
            }
            const bool on = w > 0.f;
            pv_s[tid] = on ? w : 0.f;
            y_s[tid] = on ? P.obs[(int64_t)bp * P.ld_row + (int64_t)fg * P.ld_field + c] : 0.f;
        }
        if (active) {
            f32x4 acc[2][2];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const float bv = G.bias[j * Cp + cb + sub * 16 + li];
                acc[sub][0] = f32x4{bv, bv, bv, bv};
                acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks * 32 < S) {
#pragma unroll
                    for (int sub = 0; sub < 2; ++sub) {
                        const uint4 wv = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                        mma16<__bf16>(hf[ks], wv, acc[sub][ks & 1]);
                    }
                }
            }
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
                for (int r = 0; r < 4; ++r) Vs[(sub * 16 + li) * VP + j0 + 4 * lg + r] = acc[sub][0][r] + acc[sub][1][r];
            }
        }
        __syncthreads();
        if (t + 1 < n_tiles) dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t0 + t + 1, tid);

        // b: a column per wave at a time; the lane's members' G goes to the G image (every member row below 64 V is written, the dead ones as 0)
        for (int cl = wave; cl < DM_TC; cl += NW) {
            const float pv = pv_s[cl];
            if (!(pv > 0.f)) {
                if (lane == 0) r_s[cl].state = 1;
#pragma unroll
                for (int v = 0; v < V; ++v) Gs[(lane + 64 * v) * MC_GP + cl] = Gt[(lane + 64 * v) * MC_GP + cl] = (__bf16)0.f;
                continue;
            }
            float x[V];
            double w[V], below[V];
            bool lv[V];
            const float yf = y_s[cl];
            const VfReading r = vf_score_wave_ex<V>(Vs + cl * VP, w_s, live_s, N, lane, yf, pv, x, w, below, lv);
            if (lane == 0) r_s[cl] = r;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const double g = r.state == 0 ? fwd * vf_crps_grad(x[v], w[v], below[v], lv[v], yf, cq) : 0.0;
                const float gf = (float)g;
                const __bf16 g0 = (__bf16)gf;                       // the leading term: gf rounded to bf16 once
                Gs[(lane + 64 * v) * MC_GP + cl] = g0;
                Gt[(lane + 64 * v) * MC_GP + cl] = (__bf16)(gf - (float)g0);   // what that rounding left (exact in f32), rounded to bf16: 0 where gf is a bf16 value
            }
        }
        __syncthreads();

        // c: thread k finishes column k; the waves' second product against the same tile image
        if (tid < DM_TC) {
            double tm[VF_SUMS];
            const VfReading r = r_s[tid];
            (void)vf_finish_reading(r, y_s[tid], pv_s[tid], cq, tm);
#pragma unroll
            for (int i = 0; i < VF_SUMS; ++i) term_s[i][tid] = tm[i];
        }
        if (active) {
            const uint2 glo = *reinterpret_cast<const uint2*>(Gs + (j0 + li) * MC_GP + 4 * lg);
            const uint2 ghi = *reinterpret_cast<const uint2*>(Gs + (j0 + li) * MC_GP + 16 + 4 * lg);
            const uint4 da = make_uint4(glo.x, glo.y, ghi.x, ghi.y);
            const uint2 tlo = *reinterpret_cast<const uint2*>(Gt + (j0 + li) * MC_GP + 4 * lg);
            const uint2 thi = *reinterpret_cast<const uint2*>(Gt + (j0 + li) * MC_GP + 16 + 4 * lg);
            const uint4 dt = make_uint4(tlo.x, tlo.y, thi.x, thi.y);
            const char* tbp = buf + (4 * lg + (li >> 2)) * PITCH + (4 * (li & 3)) * 2;
#pragma unroll
            for (int st = 0; st < ST; ++st) {
                if (st * 16 < S) {
                    const dm_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(tbp + st * 32));
                    const dm_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(tbp + st * 32 + 16 * PITCH));
                    const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                    const uint4 wt = make_uint4(l2.x, l2.y, h2.x, h2.y);
                    mma16<__bf16>(da, wt, dh[st]);
                    mma16<__bf16>(dt, wt, dh[st]);   // the trailing term against the same operand: a fixed order, the leading term first
                }
            }
        }
        if (t + 1 < n_tiles) dm_store_tile<SP, NT>(wr, smem + ((t + 1) & 1) * TILE, tid);
        __syncthreads();

        // d: the field's sums, columns ascending
        if (tid < VF_SUMS)
            for (int k = 0; k < DM_TC; ++k) acc_sum += term_s[tid][k];
    }
    if (tid < VF_SUMS) wsum[tid] = acc_sum;
    if (active) {   // register r of tile st is member j0 + 4 g + r, hidden column 16 st + (lane & 15)
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const int s = st * 16 + li;
            if (s < S) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int mem = j0 + 4 * lg + r;
                    if (mem < N) wpart[(int64_t)mem * S + s] = dh[st][r];
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void member_crps_finish_kernel(const MemberCrpsLaunch L, const int B) {
#pragma clang fp reassociate(off)
    const SeaDecodeMemberCrpsGrad& p = L.p;
    const int tid = threadIdx.x, N = p.members, F = p.n_fields_total, Q = L.chunks, S = p.S;
    if ((int)blockIdx.x < B) {   // the sums of history b, (patch, chunk) ascending — member_verify_finish_kernel's order — and the loss
        const int b = blockIdx.x, Pn = p.P * Q;
        const double* base = reinterpret_cast<const double*>(p.work) + (int64_t)b * Pn * F * VF_SUMS;
        for (int e = tid; e < F * VF_SUMS; e += 256) {
            const int f = e / VF_SUMS, i = e - f * VF_SUMS;
            double acc = 0.0;
#pragma unroll 8
            for (int pt = 0; pt < Pn; ++pt) acc += base[((int64_t)pt * F + f) * VF_SUMS + i];
            p.sums[((int64_t)b * F + f) * VF_SUMS + i] = acc;
            if (i == 1) {
                float fw = p.field_weight != nullptr ? p.field_weight[f] : 1.f;
                fw = fw > 0.f ? fw : 0.f;
                p.loss[(int64_t)b * F + f] = (float)((double)fw * acc);
            }
        }
        return;
    }
    const int64_t m = (int64_t)blockIdx.x - B;   // row (b N + i) P + patch
    const int patch = (int)(m % p.P);
    const int64_t bm = m / p.P;
    const int i = (int)(bm % N), b = (int)(bm / N);
    const int64_t bp = (int64_t)b * p.P + patch;
    int lim = p.C;
    if (p.counts != nullptr) {
        const int cnt = p.counts[patch];
        lim = cnt < 0 ? 0 : (cnt > p.C ? p.C : cnt);
    }
    const int tpf = (lim + DM_TC - 1) / DM_TC;
    const int qn = p.status[b] < 0 ? 0 : (tpf + MV_CHUNK - 1) / MV_CHUNK;   // the chunks that wrote a partial: [0, qn)
    const float* part = reinterpret_cast<const float*>(static_cast<const char*>(p.work) + mc_sum_bytes((int64_t)B * p.P, Q, F));
    for (int gi = 0; gi < L.n_groups; ++gi) {
        const SeaDecodeMseGroup& G = L.g[gi];
        __bf16* dH = static_cast<__bf16*>(G.dH);
        const __bf16* Z = static_cast<const __bf16*>(G.Z);
        for (int s = tid; s < S; s += 256) {
            float acc = 0.f;
            for (int jf = 0; jf < G.n_fields; ++jf)
                for (int ck = 0; ck < qn; ++ck) acc += part[((((int64_t)bp * Q + ck) * F + G.field0 + jf) * N + i) * S + s];   // (field, chunk) ascending
            if (Z != nullptr) acc *= gelu_grad_for<__bf16>((float)Z[m * G.ldz + s]);
            dH[m * G.lddh + s] = (__bf16)acc;
        }
    }
}

template <int SP, int V, int NW>
static void member_crps_launch(const MemberCrpsLaunch& L, dim3 grid, hipStream_t s) {
    constexpr int lds = mc_lds_bytes<SP>();
    static bool set_on[64] = {false};   // per device: the dynamic part is above the 64 kB a kernel gets without the attribute from SP = 384 on
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_member_crps_grad_kernel<SP, V, NW>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    decode_member_crps_grad_kernel<SP, V, NW><<<grid, dim3(64 * NW), lds, s>>>(L);
    sea_note_form(NW == 8 ? "decode.member_crps_grad.w8" : "decode.member_crps_grad.w4", SP, lds);
}

// The forms that compile without scratch (DESIGN.md section 7n has the register table): 8 waves up to SP = 384, 4 waves (members <= 64) above it;
// members above 64 beyond MC_W8_MAX_SP_V2 are refused.
constexpr int MC_W8_MAX_SP_V2 = 384;

static bool member_crps_supported(int S, int members) { return members <= 64 || S <= MC_W8_MAX_SP_V2; }

extern "C" int64_t sea_decode_member_crps_grad_ws_bytes(int B, int P, int n_fields_total, int members, int Cp, int S) {
    if (B < 1 || B > 65535 || P < 1 || n_fields_total < 1 || members < 1 || members > VF_MAX_N || Cp < 32 || Cp % 32 || S < 8 || S % 8 || S > 640) return -1;
    if (!member_crps_supported(S, members)) return -1;
    return (int64_t)B * P * mv_chunks(Cp) * n_fields_total * (VF_SUMS * 8 + (int64_t)members * S * 4);
}

// The argument checks of sea_decode_member_crps_grad and sea_decode_member_crps_grad_packed (the same struct, the same messages under the caller's name `fn`),
// in two parts, because each entry point names what it does not carry between them.
static int member_crps_check_args(const char* fn, const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberCrpsGrad* p, int dtype) {
    SEA_REQUIRE(groups != nullptr && p != nullptr, "%s: null argument table", fn);
    SEA_REQUIRE(n_groups >= 1 && n_groups <= SEA_DECODE_MSE_MAX_GROUPS, "%s: n_groups=%d outside 1..%d", fn, n_groups, SEA_DECODE_MSE_MAX_GROUPS);
    SEA_REQUIRE(dtype == SEA_F32 || dtype == SEA_BF16, "%s: bad dtype %d", fn, dtype);
    if (dtype != SEA_BF16) {
        sea_set_error("%s: unsupported: bf16 only (the fp32 decoder composes the decode and the formulas under autograd)", fn);
        return SEA_EUNSUPPORTED;
    }
    const SeaDecodeMemberCrpsGrad& P = *p;
    SEA_REQUIRE(P.obs != nullptr && P.loss != nullptr && P.sums != nullptr && P.status != nullptr && P.work != nullptr,
                "%s: null pointer (obs, loss, sums, status and work are required; prec_field, prec, field_weight, counts and logw may be NULL)", fn);
    SEA_REQUIRE(P.M >= 1, "%s: M=%d must be positive", fn, P.M);
    SEA_REQUIRE(P.S >= 8 && P.S % 8 == 0, "%s: S=%d must be a positive multiple of 8", fn, P.S);
    SEA_REQUIRE(P.Cp >= 32 && P.Cp % 32 == 0, "%s: Cp=%d must be a positive multiple of 32", fn, P.Cp);
    SEA_REQUIRE(P.C >= 1 && P.C <= P.Cp, "%s: C=%d must lie in 1..Cp=%d", fn, P.C, P.Cp);
    SEA_REQUIRE(P.P >= 1, "%s: P=%d must be positive", fn, P.P);
    SEA_REQUIRE(P.members >= 1, "%s: members=%d must be positive", fn, P.members);
    SEA_REQUIRE((int64_t)P.M % ((int64_t)P.P * P.members) == 0, "%s: M=%d is not a multiple of P * members = %d * %d", fn, P.M, P.P, P.members);
    SEA_REQUIRE(P.n_fields_total >= 1 && P.n_fields_total <= 65535, "%s: n_fields_total=%d outside 1..65535 (a grid dimension)", fn, P.n_fields_total);
    SEA_REQUIRE(P.ld_field >= P.C && P.ld_row >= 0, "%s: obs strides ld_row=%lld, ld_field=%lld must cover C=%d", fn, (long long)P.ld_row,
                (long long)P.ld_field, P.C);
    SEA_REQUIRE(P.prec == nullptr || (P.ld_pfield >= P.C && P.ld_prow >= 0), "%s: prec strides ld_prow=%lld, ld_pfield=%lld must cover C=%d", fn,
                (long long)P.ld_prow, (long long)P.ld_pfield, P.C);
    SEA_REQUIRE(P.unbiased == 0 || P.unbiased == 1, "%s: unbiased=%d must be 0 or 1", fn, P.unbiased);
    SEA_REQUIRE(sea_aligned4(P.obs) && sea_aligned4(P.prec_field) && sea_aligned4(P.prec) && sea_aligned4(P.field_weight) && sea_aligned4(P.counts) && sea_aligned4(P.logw) &&
                    sea_aligned4(P.loss) && sea_aligned4(P.status) && (reinterpret_cast<uintptr_t>(P.sums) & 7u) == 0 && (reinterpret_cast<uintptr_t>(P.work) & 7u) == 0,
                "%s: misaligned pointer (f32 and int32 buffers need 4 bytes; sums and work 8)", fn);
    int64_t covered = 0;
    for (int g = 0; g < n_groups; ++g) {
        const SeaDecodeMseGroup& G = groups[g];
        SEA_REQUIRE(G.H != nullptr && G.W2 != nullptr && G.bias != nullptr && G.dH != nullptr, "%s: group %d: null pointer (H, W2, bias or dH)", fn, g);
        SEA_REQUIRE(sea_aligned16(G.H) && sea_aligned16(G.W2) && sea_aligned16(G.bias) && sea_aligned16(G.dH) && sea_aligned16(G.Z),
                    "%s: group %d: pointers must be 16-byte aligned", fn, g);
        SEA_REQUIRE(G.ldh >= P.S && G.ldh % 8 == 0 && G.ldw >= P.S && G.ldw % 8 == 0 && G.lddh >= P.S && (G.Z == nullptr || G.ldz >= P.S),
                    "%s: group %d: row strides ldh=%d ldw=%d lddh=%d ldz=%d must cover S=%d (ldh, ldw multiples of 8)", fn, g, G.ldh, G.ldw, G.lddh, G.ldz, P.S);
        SEA_REQUIRE(G.n_fields >= 1 && G.field0 >= 0 && (int64_t)G.field0 + G.n_fields <= P.n_fields_total,
                    "%s: group %d: n_fields=%d, field0=%d outside the %d fields", fn, g, G.n_fields, G.field0, P.n_fields_total);
        SEA_REQUIRE((int64_t)G.n_fields * P.Cp <= 0x7fffffffLL / 2, "%s: group %d: too many output columns", fn, g);
        for (int h = 0; h < g; ++h)
            SEA_REQUIRE(G.field0 >= groups[h].field0 + groups[h].n_fields || groups[h].field0 >= G.field0 + G.n_fields,
                        "%s: group %d: its fields overlap those of group %d (a cell is scored once)", fn, g, h);
        covered += G.n_fields;
    }
    SEA_REQUIRE(covered == P.n_fields_total, "%s: the groups cover %lld of the %d fields (every field needs exactly one group)", fn, (long long)covered,
                P.n_fields_total);
    return SEA_OK;
}

static int member_crps_check_size(const char* fn, const SeaDecodeMemberCrpsGrad& P, int64_t* B_out, int* Q_out) {
    const int64_t BP = (int64_t)P.M / P.members;
    const int64_t B = BP / P.P;
    SEA_REQUIRE(BP <= 0x7fffffffLL && B <= 65535, "%s: %lld histories; a launch carries up to 65535", fn, (long long)B);
    const int Q = mv_chunks(P.Cp);
    SEA_REQUIRE(Q <= 65535 && B + (int64_t)P.M <= 0x7fffffffLL, "%s: too many rows or column chunks", fn);
    const int64_t need = sea_decode_member_crps_grad_ws_bytes((int)B, P.P, P.n_fields_total, P.members, P.Cp, P.S);
    SEA_REQUIRE(P.work_bytes >= need,
                "%s: work_bytes=%lld below the %lld that sea_decode_member_crps_grad_ws_bytes(B=%d, P=%d, n_fields_total=%d, members=%d, Cp=%d, S=%d) asks for", fn,
                (long long)P.work_bytes, (long long)need, (int)B, P.P, P.n_fields_total, P.members, P.Cp, P.S);
    *B_out = B;
    *Q_out = Q;
    return SEA_OK;
}

extern "C" int sea_decode_member_crps_grad(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberCrpsGrad* p, int dtype, void* stream) {
    const int rc = member_crps_check_args("sea_decode_member_crps_grad", groups, n_groups, p, dtype);
    if (rc != SEA_OK) return rc;
    const SeaDecodeMemberCrpsGrad& P = *p;
    if (P.S > 640) {
        sea_set_error("sea_decode_member_crps_grad: unsupported: hidden width S=%d above 640", P.S);
        return SEA_EUNSUPPORTED;
    }
    if (P.members > VF_MAX_N) {
        sea_set_error("sea_decode_member_crps_grad: unsupported: members=%d above %d", P.members, VF_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    if (!member_crps_supported(P.S, P.members)) {
        sea_set_error("sea_decode_member_crps_grad: unsupported: members=%d above 64 at hidden width S=%d above %d (the dH slice and the two-member walk do not fit the register file)",
                      P.members, P.S, MC_W8_MAX_SP_V2);
        return SEA_EUNSUPPORTED;
    }
    int64_t B = 0;
    int Q = 0;
    const int rs = member_crps_check_size("sea_decode_member_crps_grad", P, &B, &Q);
    if (rs != SEA_OK) return rs;

    MemberCrpsLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    L.n_groups = n_groups;
    L.chunks = Q;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(B * P.P), (unsigned)P.n_fields_total, (unsigned)Q);
    const int S = P.S;
    if (P.members > 64) {
        if (S <= 128) member_crps_launch<128, 2, 8>(L, grid, s);
        else if (S <= 256) member_crps_launch<256, 2, 8>(L, grid, s);
        else member_crps_launch<384, 2, 8>(L, grid, s);
    } else {
        if (S <= 128) member_crps_launch<128, 1, 8>(L, grid, s);
        else if (S <= 256) member_crps_launch<256, 1, 8>(L, grid, s);
        else if (S <= 384) member_crps_launch<384, 1, 8>(L, grid, s);
        else if (S <= 512) member_crps_launch<512, 1, 4>(L, grid, s);
        else member_crps_launch<640, 1, 4>(L, grid, s);
    }
    member_crps_finish_kernel<<<dim3((unsigned)(B + P.M)), dim3(256), 0, s>>>(L, (int)B);
    SEA_CHECK_LAUNCH("sea_decode_member_crps_grad");
    return SEA_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------------
// sea_decode_member_crps_grad_packed: sea_decode_member_crps_grad's launch 1 for 1 .. 32 members, several HISTORIES per workgroup (include/sea_hip.h;
// DESIGN.md section 7n).  At 4 members the unpacked form decodes 4 real rows of a 16-row MFMA tile, scores with 4 of 64 lanes and pays the tile loads,
// the barriers and the 32 wave-passes of a tile for them.  Here a workgroup serves (a group of HG histories, patch, field, chunk): with NP the member
// count rounded up to a power of two (at least 2), slot g NP + i of 64 is member i of the group's history g, HG = 64 / NP (less where LDS does not
// admit it: mcp_groups).  Waves 0 - 3 decode 16 slots each with the unpacked form's MFMA sequence into Vs[column][slot]; per column a wave scores all
// the group's histories at once (vf_score_seg_ex<NP>: segments of NP lanes), each lane forms its G with ITS history's c and rounds it to the two bf16
// terms at its slot's row of the G images, and the segment's first lane finishes the reading (vf_finish_reading) and files its eight terms; the second
// product multiplies the slot rows' G fragments against the same tile image; thread (g, i) adds sum i of history g, columns ascending, one chain per
// history across the tiles.  The per-history setup (log-weights, live flags, w, q, c, status) is the unpacked kernel's statements with the same
// j-ascending chains, run by the history's own slot threads.  A history that is not scored and a history index >= B in the last group are dead
// segments by selects: no cell of theirs has weight, so they write zero sums and nothing else; the workgroup leaves early only when none of its
// histories has anything to score.  Outputs go to the unpacked form's workspace slots ((b P + p) Q + ck) F + f, and member_crps_finish_kernel runs
// unchanged as launch 2.  The bits are the unpacked form's: an MFMA row does not depend on the other rows of its tile, a segment's butterflies pair as
// the whole wave's do (verify_score.hpp), and every chain of a history is the same chain — one writer per element, no floating-point atomics, nothing
// of a history depends on another.
// LDS: the term staging [32 columns][HG][8] fp64 is 64 KiB at HG = 32; beside the 640-wide tile images that is above a CU's 160 KiB, so that one
// instantiation (SP = 640, NP = 2) runs HG = 16 (slots 0 .. 31, waves 0 and 1 decode); every other one has HG = 64 / NP.
constexpr int MCP_VP = 65;        // floats per column of the packed value image: 64 slots and one of pad
constexpr int MCP_STATIC = 2560;  // bound on the kernel's static LDS (the per-slot and per-segment setup arrays and the barriers' words: at most 2176 bytes)

template <int SP, int HG>
constexpr int mcp_lds_bytes() { return 2 * DM_TC * (SP * 2 + DM_PAD) + DM_TC * MCP_VP * 4 + 2 * 64 * MC_GP * 2 + HG * DM_TC * (VF_SUMS * 8 + 2 * 4); }

template <int SP, int NP>
constexpr int mcp_groups() { return (SP > 512 && NP == 2) ? 16 : 64 / NP; }

template <int SP, int NP, int NW, int HG>
__global__ __launch_bounds__(64 * NW) void decode_member_crps_pack_kernel(const MemberCrpsLaunch L, const int B) {
#pragma clang fp reassociate(off)
    constexpr int NT = 64 * NW;
    constexpr int KS = SP / 32;
    constexpr int ST = SP / 16;
    constexpr int PITCH = SP * 2 + DM_PAD;
    constexpr int TILE = DM_TC * PITCH;
    constexpr int NCH = SP * 4 / NT;
    constexpr int VP = MCP_VP;
    constexpr int SEG = 64 / NP;
    static_assert(NCH * NT == DM_TC * (SP / 8), "whole chunks per thread");
    static_assert(HG >= 1 && HG <= SEG, "a group's slots fit one wave");
    static_assert(NT >= HG * VF_SUMS, "a thread per (history, sum)");
    static_assert(mcp_lds_bytes<SP, HG>() + MCP_STATIC <= 160 * 1024, "the tile images, the value and G images and the per-(history, column) staging fit a CU's LDS");
    extern __shared__ __attribute__((aligned(16))) char smem[];   // 2 tile images; the value image [32][VP]; the two G images [64][MC_GP]; terms [32][HG][8]; y, pv [HG][32]
    float* Vs = reinterpret_cast<float*>(smem + 2 * TILE);
    __bf16* Gs = reinterpret_cast<__bf16*>(smem + 2 * TILE + DM_TC * VP * 4);
    __bf16* Gt = Gs + 64 * MC_GP;
    double* term_s = reinterpret_cast<double*>(smem + 2 * TILE + DM_TC * VP * 4 + 2 * 64 * MC_GP * 2);
    float* y_s = reinterpret_cast<float*>(term_s + DM_TC * HG * VF_SUMS);
    float* pv_s = y_s + HG * DM_TC;
    __shared__ double lw_s[64], w_s[64], cq_s[SEG];
    __shared__ int live_s[64], inv_s[64], ok_s[SEG];
    static_assert(sizeof(double) * (128 + SEG) + sizeof(int) * (128 + SEG) <= MCP_STATIC, "MCP_STATIC bounds the static arrays");

    const SeaDecodeMemberCrpsGrad& P = L.p;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), li = lane & 15, lg = lane >> 4;
    const int S = P.S, C = P.C, Cp = P.Cp, N = P.members, F = P.n_fields_total;
    const int fg = blockIdx.y, ck = blockIdx.z, Q = gridDim.z;
    const int grp = blockIdx.x / P.P, patch = blockIdx.x - grp * P.P;
    const int b0 = grp * HG;                              // the group's first history
    const int nh = B - b0 < HG ? B - b0 : HG;             // its histories: [b0, b0 + nh)
    char* const wpart0 = static_cast<char*>(P.work) + mc_sum_bytes((int64_t)B * P.P, Q, F);
    auto ws_slot = [&](int g) { return (((int64_t)(b0 + g) * P.P + patch) * Q + ck) * F + fg; };   // history b0 + g's place in both parts of the workspace

    int lim = C;   // valid columns of this patch: [0, lim) — uniform over the workgroup
    if (P.counts != nullptr) {
        const int cnt = P.counts[patch];
        lim = cnt < 0 ? 0 : (cnt > C ? C : cnt);
    }
    const int tpf = (lim + DM_TC - 1) / DM_TC;
    const int tb = ck * MV_CHUNK, te = tpf < tb + MV_CHUNK ? tpf : tb + MV_CHUNK;

    // the weights of the group's histories: the unpacked kernel's statements, thread `tid` < 64 as member si of segment sg (its chains run over its own segment)
    const int si = tid & (NP - 1), sg = (tid & 63) / NP, sbase = (tid & 63) - si;
    const bool slot_t = tid < 64;
    const bool member = slot_t && sg < nh && si < N;
    int invalid = 0, alive = 0;
    if (slot_t) {
        const float lw = (member && P.logw != nullptr) ? P.logw[(int64_t)(b0 + sg) * N + si] : 0.f;
        invalid = (member && (lw != lw || lw == INFINITY)) ? 1 : 0;
        alive = (member && !invalid && lw != -INFINITY) ? 1 : 0;
        lw_s[tid] = (double)lw;
        live_s[tid] = alive;
        inv_s[tid] = invalid;
    }
    __syncthreads();
    int ok = 0;
    if (slot_t) {
        int n_live = 0, inv = 0;
        for (int j = 0; j < N; ++j) {
            n_live += live_s[sbase + j];
            inv |= inv_s[sbase + j];
        }
        ok = (sg < nh && !inv && n_live > 0) ? 1 : 0;   // the history is scored
        if (si == 0) {
            ok_s[sg] = ok;
            if (sg < nh && patch == 0 && fg == 0 && ck == 0) P.status[b0 + sg] = ok ? n_live : -1;
        }
    }
    const int any_ok = __syncthreads_or(ok);
    if (!any_ok || te <= tb) {   // uniform: nothing to score in this chunk for any history of the group; the finish launch passes their partials over
        if (tid < HG * VF_SUMS && (tid >> 3) < nh) (reinterpret_cast<double*>(P.work) + ws_slot(tid >> 3) * VF_SUMS)[tid & 7] = 0.0;
        return;
    }
    if (slot_t) {
        double mx = -INFINITY;
        for (int j = 0; j < N; ++j) mx = lw_s[sbase + j] > mx ? lw_s[sbase + j] : mx;
        w_s[tid] = (alive && ok) ? exp(lw_s[tid] - mx) : 0.0;
    }
    __syncthreads();
    double my_w = 0.0;
    if (slot_t) {
        double W = 0.0;
        for (int j = 0; j < N; ++j) W += w_s[sbase + j];
        my_w = (member && ok) ? w_s[tid] / W : 0.0;
    }
    __syncthreads();
    if (slot_t) w_s[tid] = my_w;
    __syncthreads();
    if (slot_t) {
        double q = 0.0;
        for (int j = 0; j < N; ++j) q = fma(w_s[sbase + j], w_s[sbase + j], q);
        if (si == 0) cq_s[sg] = P.unbiased ? 1.0 - q : 1.0;
    }
    __syncthreads();
    float fwv = P.field_weight != nullptr ? P.field_weight[fg] : 1.f;
    fwv = fwv > 0.f ? fwv : 0.f;   // false for NaN
    const double fwd = (double)fwv;

    // the scoring lane: member lane & (NP - 1) of segment lane / NP
    const int lseg = lane / NP;
    const int gs = lseg < HG ? lseg : 0;
    const bool seg_on = lseg < HG && ok_s[gs] != 0;
    const bool lead = lseg < HG && (lane & (NP - 1)) == 0;
    const double cq = cq_s[lseg];

    // the decoding lane: slot j0 + li
    const int j0 = wave * 16;
    const bool active = j0 < nh * NP;
    const int dg = (j0 + li) / NP, di = (j0 + li) & (NP - 1);
    const bool dvalid = dg < nh && di < N;
    const int64_t m = ((int64_t)(b0 + (dvalid ? dg : 0)) * N + (dvalid ? di : 0)) * P.P + patch;
    double acc_sum = 0.0;

    int gsel = 0;
    for (int gi = 1; gi < L.n_groups; ++gi) gsel = (fg >= L.g[gi].field0 && fg < L.g[gi].field0 + L.g[gi].n_fields) ? gi : gsel;
    const SeaDecodeMseGroup& G = L.g[gsel];
    const int j = fg - G.field0;
    const __bf16* H = static_cast<const __bf16*>(G.H);
    const __bf16* W2 = static_cast<const __bf16*>(G.W2);
    uint4 hf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        const int s = ks * 32 + 8 * lg;
        if (ks * 32 + 32 <= S) {
            hf[ks] = *reinterpret_cast<const uint4*>(H + m * G.ldh + s);
        } else {
            const uint4 v = *reinterpret_cast<const uint4*>(H + m * G.ldh + (s < S ? s : 0));
            hf[ks] = s < S ? v : make_uint4(0u, 0u, 0u, 0u);
        }
    }
    f32x4 dh[ST];
#pragma unroll
    for (int st = 0; st < ST; ++st) dh[st] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int n_tiles = te - tb, t0 = j * tpf + tb;
    uint4 wr[NCH];
    dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t0, tid);
    dm_store_tile<SP, NT>(wr, smem, tid);
    __syncthreads();

    typedef dm_s16x4 __attribute__((address_space(3))) * lds_p;
    for (int t = 0; t < n_tiles; ++t) {
        const char* buf = smem + (t & 1) * TILE;
        const int cb = (tb + t) * DM_TC;

        // a: per (history, column) the cell's weight and reading (a history that is not scored: no weight); decode into the value image
        for (int e = tid; e < HG * DM_TC; e += NT) {
            const int g = e >> 5, c = cb + (e & 31);
            const int64_t bpg = (int64_t)(b0 + g) * P.P + patch;
            float w = 0.f;
            if (c < lim && ok_s[g] != 0) {
                const float pf = P.prec_field != nullptr ? P.prec_field[fg] : 1.f;
                const float pm = P.prec != nullptr ? P.prec[bpg * P.ld_prow + (int64_t)fg * P.ld_pfield + c] : 1.f;
                w = mul1(pf > 0.f ? pf : 0.f, pm > 0.f ? pm : 0.f);
            }
            const bool on = w > 0.f;
            pv_s[e] = on ? w : 0.f;
            y_s[e] = on ? P.obs[bpg * P.ld_row + (int64_t)fg * P.ld_field + c] : 0.f;
        }
        if (active) {
            f32x4 acc[2][2];
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                const float bv = G.bias[j * Cp + cb + sub * 16 + li];
                acc[sub][0] = f32x4{bv, bv, bv, bv};
                acc[sub][1] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if (ks * 32 < S) {
#pragma unroll
                    for (int sub = 0; sub < 2; ++sub) {
                        const uint4 wv = *reinterpret_cast<const uint4*>(buf + (sub * 16 + li) * PITCH + (ks * 4 + lg) * 16);
                        mma16<__bf16>(hf[ks], wv, acc[sub][ks & 1]);
                    }
                }
            }
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
#pragma unroll
                for (int r = 0; r < 4; ++r) Vs[(sub * 16 + li) * VP + j0 + 4 * lg + r] = acc[sub][0][r] + acc[sub][1][r];
            }
        }
        __syncthreads();
        if (t + 1 < n_tiles) dm_load_tile<SP, NT>(wr, W2, G.ldw, S, Cp, tpf, t0 + t + 1, tid);

        // b: a column per wave at a time, all the group's histories at once; the lane's G goes to its slot's row of the G images (every row is written,
        //    the dead ones as 0) and the segment's first lane finishes the reading and files its terms
        for (int cl = wave; cl < DM_TC; cl += NW) {
            const float pv = seg_on ? pv_s[gs * DM_TC + cl] : 0.f;
            const float yf = seg_on ? y_s[gs * DM_TC + cl] : 0.f;
            const bool on = pv > 0.f;
            if (__ballot(on) == 0) {   // uniform: the cell is dead in every history
                Gs[lane * MC_GP + cl] = Gt[lane * MC_GP + cl] = (__bf16)0.f;
                if (lead) {
#pragma unroll
                    for (int i = 0; i < VF_SUMS; ++i) term_s[(cl * HG + gs) * VF_SUMS + i] = 0.0;
                }
                continue;
            }
            float x;
            double w, below;
            bool lv;
            VfReading r = vf_score_seg_ex<NP>(Vs + cl * VP, w_s, live_s, N, lane, seg_on, yf, pv, x, w, below, lv);
            r.state = on ? r.state : 1;   // a segment whose cell is dead
            {
                const double g = r.state == 0 ? fwd * vf_crps_grad(x, w, below, lv, yf, cq) : 0.0;
                const float gf = (float)g;
                const __bf16 g0 = (__bf16)gf;                       // the leading term: gf rounded to bf16 once
                Gs[lane * MC_GP + cl] = g0;
                Gt[lane * MC_GP + cl] = (__bf16)(gf - (float)g0);   // what that rounding left (exact in f32), rounded to bf16: 0 where gf is a bf16 value
            }
            double tm[VF_SUMS];
            (void)vf_finish_reading(r, yf, pv, cq, tm);
            if (lead) {
#pragma unroll
                for (int i = 0; i < VF_SUMS; ++i) term_s[(cl * HG + gs) * VF_SUMS + i] = tm[i];
            }
        }
        __syncthreads();

        // c: the waves' second product against the same tile image
        if (active) {
            const uint2 glo = *reinterpret_cast<const uint2*>(Gs + (j0 + li) * MC_GP + 4 * lg);
            const uint2 ghi = *reinterpret_cast<const uint2*>(Gs + (j0 + li) * MC_GP + 16 + 4 * lg);
            const uint4 da = make_uint4(glo.x, glo.y, ghi.x, ghi.y);
            const uint2 tlo = *reinterpret_cast<const uint2*>(Gt + (j0 + li) * MC_GP + 4 * lg);
            const uint2 thi = *reinterpret_cast<const uint2*>(Gt + (j0 + li) * MC_GP + 16 + 4 * lg);
            const uint4 dt = make_uint4(tlo.x, tlo.y, thi.x, thi.y);
            const char* tbp = buf + (4 * lg + (li >> 2)) * PITCH + (4 * (li & 3)) * 2;
#pragma unroll
            for (int st = 0; st < ST; ++st) {
                if (st * 16 < S) {
                    const dm_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(tbp + st * 32));
                    const dm_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(tbp + st * 32 + 16 * PITCH));
                    const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                    const uint4 wt = make_uint4(l2.x, l2.y, h2.x, h2.y);
                    mma16<__bf16>(da, wt, dh[st]);
                    mma16<__bf16>(dt, wt, dh[st]);   // the trailing term against the same operand: a fixed order, the leading term first
                }
            }
        }
        if (t + 1 < n_tiles) dm_store_tile<SP, NT>(wr, smem + ((t + 1) & 1) * TILE, tid);
        __syncthreads();

        // d: thread (g, i): sum i of history g, columns ascending
        if (tid < HG * VF_SUMS)
            for (int k = 0; k < DM_TC; ++k) acc_sum += term_s[k * HG * VF_SUMS + tid];
    }
    if (tid < HG * VF_SUMS && (tid >> 3) < nh) (reinterpret_cast<double*>(P.work) + ws_slot(tid >> 3) * VF_SUMS)[tid & 7] = acc_sum;
    if (active) {   // register r of tile st is slot j0 + 4 g + r, hidden column 16 st + (lane & 15); a history that is not scored writes no partial
        float* wrow[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int slot = j0 + 4 * lg + r, g = slot / NP, i = slot & (NP - 1);
            const bool wv = g < nh && i < N && ok_s[g < SEG ? g : 0] != 0;
            wrow[r] = wv ? reinterpret_cast<float*>(wpart0) + (ws_slot(g) * N + i) * S : nullptr;
        }
#pragma unroll
        for (int st = 0; st < ST; ++st) {
            const int s = st * 16 + li;
            if (s < S) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (wrow[r] != nullptr) wrow[r][s] = dh[st][r];
            }
        }
    }
}

template <int SP, int NP, int NW>
static void member_crps_pack_launch(const MemberCrpsLaunch& L, int B, hipStream_t s) {
    constexpr int HG = mcp_groups<SP, NP>();
    constexpr int lds = mcp_lds_bytes<SP, HG>();
    static bool set_on[64] = {false};   // per device: the dynamic part is above the 64 kB a kernel gets without the attribute in most instantiations
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !set_on[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(decode_member_crps_pack_kernel<SP, NP, NW, HG>), hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (dev >= 0) set_on[dev] = true;
    }
    const dim3 grid((unsigned)(((B + HG - 1) / HG) * L.p.P), (unsigned)L.p.n_fields_total, (unsigned)L.chunks);
    decode_member_crps_pack_kernel<SP, NP, NW, HG><<<grid, dim3(64 * NW), lds, s>>>(L, B);
    // the form's name carries NP; the histories per workgroup are 64 / NP, except "pk2h16" (S above 512 at 1 or 2 members: 16)
    sea_note_form(NP == 2 ? (HG == 32 ? "decode.member_crps_grad.pk2" : "decode.member_crps_grad.pk2h16")
                          : NP == 4 ? "decode.member_crps_grad.pk4" : NP == 8 ? "decode.member_crps_grad.pk8" : NP == 16 ? "decode.member_crps_grad.pk16" : "decode.member_crps_grad.pk32",
                  SP, lds);
}

template <int NP>
static void member_crps_pack_dispatch(const MemberCrpsLaunch& L, int B, hipStream_t s) {
    const int S = L.p.S;
    if (S <= 128) member_crps_pack_launch<128, NP, 8>(L, B, s);
    else if (S <= 256) member_crps_pack_launch<256, NP, 8>(L, B, s);
    else if (S <= 384) member_crps_pack_launch<384, NP, 8>(L, B, s);
    else if (S <= 512) member_crps_pack_launch<512, NP, 4>(L, B, s);
    else member_crps_pack_launch<640, NP, 4>(L, B, s);
}

constexpr int MCP_MAX_N = 32;   // the packed form's member counts: 1 .. 32 (above: one history fills most of a wave; the unpacked form serves)

// Every (S, NP) up to S = 640 compiles without scratch (DESIGN.md section 7n has the table), so nothing below MCP_MAX_N members is refused.
static bool member_crps_pack_supported(int S, int members) { return members >= 1 && members <= MCP_MAX_N && S <= 640; }

extern "C" int sea_decode_member_crps_grad_packed(const SeaDecodeMseGroup* groups, int n_groups, const SeaDecodeMemberCrpsGrad* p, int dtype, void* stream) {
    const int rc = member_crps_check_args("sea_decode_member_crps_grad_packed", groups, n_groups, p, dtype);
    if (rc != SEA_OK) return rc;
    const SeaDecodeMemberCrpsGrad& P = *p;
    if (P.S > 640) {
        sea_set_error("sea_decode_member_crps_grad_packed: unsupported: hidden width S=%d above 640", P.S);
        return SEA_EUNSUPPORTED;
    }
    if (P.members > MCP_MAX_N) {
        sea_set_error("sea_decode_member_crps_grad_packed: unsupported: members=%d above %d (the packed form serves 1 .. %d members; sea_decode_member_crps_grad serves above)",
                      P.members, MCP_MAX_N, MCP_MAX_N);
        return SEA_EUNSUPPORTED;
    }
    if (!member_crps_pack_supported(P.S, P.members)) {
        sea_set_error("sea_decode_member_crps_grad_packed: unsupported: members=%d at hidden width S=%d is not shipped", P.members, P.S);
        return SEA_EUNSUPPORTED;
    }
    int64_t B = 0;
    int Q = 0;
    const int rs = member_crps_check_size("sea_decode_member_crps_grad_packed", P, &B, &Q);
    if (rs != SEA_OK) return rs;

    MemberCrpsLaunch L;
    memset(&L, 0, sizeof(L));
    for (int g = 0; g < n_groups; ++g) L.g[g] = groups[g];
    L.p = P;
    L.n_groups = n_groups;
    L.chunks = Q;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int n = P.members;
    if (n <= 2) member_crps_pack_dispatch<2>(L, (int)B, s);
    else if (n <= 4) member_crps_pack_dispatch<4>(L, (int)B, s);
    else if (n <= 8) member_crps_pack_dispatch<8>(L, (int)B, s);
    else if (n <= 16) member_crps_pack_dispatch<16>(L, (int)B, s);
    else member_crps_pack_dispatch<32>(L, (int)B, s);
    member_crps_finish_kernel<<<dim3((unsigned)(B + P.M)), dim3(256), 0, s>>>(L, (int)B);
    SEA_CHECK_LAUNCH("sea_decode_member_crps_grad_packed");
    return SEA_OK;
}
