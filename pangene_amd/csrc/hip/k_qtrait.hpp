// ------------------------------------------------------------------------------------------------
// Quantitative traits (pga_pan_qtrait; DESIGN.md section 8 "Quantitative traits"): the rank-sum permutation test of one trait against
// every gene.  With N columns, c2 the centred doubled midranks (sum c2 = 0, |c2| <= N - 1 <= 31 999), a = |B_g| and
// D = sum of c2 over the columns of B_g: permutation p gives c2_p[r] = c2[o_p[r]], D_p = sum of c2_p over B_g, and k_g counts the p with
// |D_p| >= |D|.  Over all genes and permutations D_p is the integer matrix product B[G][N] . C^T[N][n]: the first kernel of this
// project on the matrix cores.
//   obs    k_qtrait_obs: a and D of every row (8 lanes a row, as k_trait_obs: a lane walks the set bits of its words) and the threshold
//          absD = |D|, INT32_MAX for a row that is not eligible: |D_p| <= N (N - 1) / 2 < 2^30 never reaches it.
//   perm   k_qtrait_perm: the value rows of one batch of permutations.  One lane per permutation runs the pinned swap sequence
//          (k_perm.hpp) over a private int16 row and swaps the two values.  The wave's 64 rows are laid out as k_perm.hpp says, in LDS
//          while they fit (N <= 256) and in a global scratch buffer beyond.  A finished row is written as two signed-byte digit planes
//          lo[nb][K], hi[nb][K] with
//          lo = ((c2 + 128) & 255) - 128 in [-128, 127] and hi = (c2 - lo) >> 8 in [-125, 125], c2 = 256 hi + lo; K = N rounded up
//          to QT_KC, the columns past N written as zero.
//   count  k_qtrait_count: an int8 GEMM on v_mfma_i32_16x16x64_i8.  One workgroup of four waves per 128 genes x 128 permutations,
//          each wave 64 x 64 as 4 x 4 MFMA tiles, one accumulator set per digit plane (the hi set and its loads are left out when
//          N <= 128: every hi is 0 there).  Per chunk of QT_KC = 128 columns the gene BITS are expanded to 0/1 bytes on their way
//          into LDS -- the bit matrix is the only copy of B in HBM -- and the two planes are copied as they are; rows are
//          QT_LD = 144 bytes apart, so the 16 rows a ds_read_b128 of an operand touches start in 16 distinct groups of four banks.
//          The operand maps: lane l holds, for A, row l & 15 and, for B, column l & 15, both over the same 16 bytes
//          k = 16 (l >> 4) .. + 15 of the 64-column step.  A and B share the (lane, byte) -> k map and the sum over k does not care
//          about its order, so only the row / column side has to be right; the result map is the one every 16 x 16 MFMA has,
//          column = l & 15 (permutation), row = 4 (l >> 4) + register (gene).  Epilogue: D_p = 256 acc_hi + acc_lo, |D_p| against the
//          row's absD with the permutations past the batch masked, the hits of a gene summed over a wave's 64 permutations (four
//          tiles in the lane, then four __shfl_xor over the 16 lanes that share the gene), ONE atomicAdd per (wave tile, gene) with a
//          hit into k[g].  Integer adds commute, so k does not depend on scheduling.
// ------------------------------------------------------------------------------------------------
constexpr int32_t QT_ROW_LANES = 8;      // lanes that share one row in k_qtrait_obs (row8_sum)
constexpr int32_t QT_PERM_LDS_N = 256;   // columns up to which a wave's 64 int16 rows stay in LDS (32 KiB)
constexpr int32_t QT_NEVER = 0x7fffffff; // the threshold of a row that is not eligible
constexpr int32_t QT_TILE = 128;         // genes and permutations of a workgroup's tile
constexpr int32_t QT_KC = 128;           // columns of a K chunk: two MFMA steps of 64
constexpr int32_t QT_LD = QT_KC + 16;    // bytes between the rows of a staged tile
constexpr int32_t QT_HI_FROM = 129;      // N from which a hi digit can be nonzero (|c2| <= N - 1 >= 128)

typedef int32_t qt_v4i __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(BLOCK) void k_qtrait_obs(const uint32_t *__restrict__ bits, const int16_t *__restrict__ c2, int32_t G, int32_t W, int32_t N,
                                                      int32_t min_count, int32_t *__restrict__ a_out, int32_t *__restrict__ d_out, int32_t *__restrict__ abs_out)
{
	const int64_t g = (int64_t)blockIdx.x * (BLOCK / QT_ROW_LANES) + (int64_t)(threadIdx.x / QT_ROW_LANES);
	const int32_t l = (int32_t)threadIdx.x % QT_ROW_LANES;
	int32_t a = 0, d = 0;
	if (g < G) {
		const uint32_t *row = bits + (size_t)g * (size_t)W;
		for (int32_t k = l; k < W; k += QT_ROW_LANES) {
			uint32_t w = row[k];
			a += __popc(w);
			for (; w; w &= w - 1) d += (int32_t)c2[k * 32 + __ffs((int32_t)w) - 1]; // (bits past N are zero)
		}
	}
	a = row8_sum(a), d = row8_sum(d);
	if (g < G && l == 0) a_out[g] = a, d_out[g] = d, abs_out[g] = min(a, N - a) >= min_count ? (d < 0 ? -d : d) : QT_NEVER;
}

// perm_wave_rows (k_perm.hpp) over rows of N values: permutation p0 + q of the batch is row q of lo[nb][K] and hi[nb][K].  USE_LDS:
// the wave's rows in LDS; otherwise in work[workgroup][N][64].
template <bool USE_LDS>
__global__ __launch_bounds__(WAVE) void k_qtrait_perm(const int16_t *__restrict__ c2, int32_t N, int32_t K, uint32_t seed, uint32_t p0, int32_t nb,
                                                      int16_t *__restrict__ work, int8_t *__restrict__ lo, int8_t *__restrict__ hi)
{
	perm_wave_rows<int16_t, QT_PERM_LDS_N, USE_LDS>(
		N, N, seed, p0, nb, work, [&](int32_t c) { return c2[c]; }, PermSwapValues(),
		[&](const int16_t *fin, int64_t q, int32_t l) { // four columns a lane: one 32-bit store per plane (K is a multiple of 4)
			uint32_t *out_lo = (uint32_t *)(lo + (size_t)q * (size_t)K), *out_hi = (uint32_t *)(hi + (size_t)q * (size_t)K);
			for (int32_t c = 4 * l; c < K; c += 4 * WAVE) {
				uint32_t wl = 0, wh = 0;
#pragma unroll
				for (int32_t e = 0; e < 4; ++e) {
					const int32_t v = c + e < N ? (int32_t)fin[(c + e) * WAVE] : 0;
					const int32_t dl = ((v + 128) & 255) - 128, dh = (v - dl) >> 8;
					wl |= (uint32_t)(dl & 255) << (8 * e), wh |= (uint32_t)(dh & 255) << (8 * e);
				}
				out_lo[c >> 2] = wl, out_hi[c >> 2] = wh;
			}
		});
}

// four bits -> four 0/1 bytes, bit e in byte e (the products of the multiplication share no bit, so nothing carries)
__device__ __forceinline__ uint32_t qt_nibble_bytes(uint32_t x) { return ((x & 15u) * 0x00204081u) & 0x01010101u; }

// grid: (ceil(G / 128), ceil(nb / 128)).  bits[G][W], lo / hi[nb][K] with K a multiple of QT_KC and 16-byte aligned rows, absd[G];
// k[g] += hits.  d_rows: NULL, or (tests) d_rows[p][g] = D_p of the batch's permutation p, [nb][G].
template <bool HI>
__global__ __launch_bounds__(BLOCK, 2) void k_qtrait_count(const uint32_t *__restrict__ bits, const int8_t *__restrict__ lo, const int8_t *__restrict__ hi,
                                                        const int32_t *__restrict__ absd, int32_t G, int32_t nb, int32_t W, int32_t K,
                                                        int32_t *__restrict__ k_out, int32_t *__restrict__ d_rows)
{
	__shared__ uint4 sh_g[QT_TILE * QT_LD / 16], sh_lo[QT_TILE * QT_LD / 16], sh_hi[HI ? QT_TILE * QT_LD / 16 : 1];
	const int32_t t = (int32_t)threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
	const int32_t i0 = (int32_t)blockIdx.x * QT_TILE, j0 = (int32_t)blockIdx.y * QT_TILE;
	const int32_t wi = (wv >> 1) * 64, wj = (wv & 1) * 64; // the wave's 64 x 64 corner in the tile
	const int32_t fr = lane & 15, fk = (lane >> 4) * 16;   // operand fragment: row / column, first byte of the step

	qt_v4i acc_lo[4][4], acc_hi[HI ? 4 : 1][HI ? 4 : 1];
#pragma unroll
	for (int32_t m = 0; m < 4; ++m)
#pragma unroll
		for (int32_t n = 0; n < 4; ++n) {
			acc_lo[m][n] = qt_v4i{0, 0, 0, 0};
			if constexpr (HI) acc_hi[m][n] = qt_v4i{0, 0, 0, 0};
		}

	// staging: thread t expands words 2 (t & 1), + 1 of gene row t >> 1 (64 columns) and copies 16 bytes x 4 of each plane
	const int32_t sg_row = t >> 1, sg_half = t & 1;
	const bool sg_ok = i0 + sg_row < G;
	const uint32_t *sg_src = bits + (size_t)(sg_ok ? i0 + sg_row : 0) * (size_t)W;
	for (int32_t k0 = 0; k0 < K; k0 += QT_KC) {
		{
			const int32_t w0 = (k0 >> 5) + 2 * sg_half;
			const uint32_t b0 = sg_ok && w0 < W ? sg_src[w0] : 0u, b1 = sg_ok && w0 + 1 < W ? sg_src[w0 + 1] : 0u;
			uint4 *dst = sh_g + (sg_row * QT_LD + sg_half * 64) / 16;
#pragma unroll
			for (int32_t q = 0; q < 2; ++q) {
				const uint32_t b = q ? b1 : b0;
				dst[2 * q] = make_uint4(qt_nibble_bytes(b), qt_nibble_bytes(b >> 4), qt_nibble_bytes(b >> 8), qt_nibble_bytes(b >> 12));
				dst[2 * q + 1] = make_uint4(qt_nibble_bytes(b >> 16), qt_nibble_bytes(b >> 20), qt_nibble_bytes(b >> 24), qt_nibble_bytes(b >> 28));
			}
		}
#pragma unroll
		for (int32_t q = 0; q < 4; ++q) {
			const int32_t idx = t + BLOCK * q, row = idx >> 3, seg = idx & 7;
			const bool ok = j0 + row < nb; // rows past the batch: zero (they are masked in the epilogue too)
			const size_t at = (size_t)(ok ? j0 + row : 0) * (size_t)K + (size_t)(k0 + seg * 16);
			sh_lo[(row * QT_LD + seg * 16) / 16] = ok ? *(const uint4 *)(lo + at) : make_uint4(0, 0, 0, 0);
			if constexpr (HI) sh_hi[(row * QT_LD + seg * 16) / 16] = ok ? *(const uint4 *)(hi + at) : make_uint4(0, 0, 0, 0);
		}
		__syncthreads();
#pragma unroll
		for (int32_t ks = 0; ks < QT_KC; ks += 64) {
			qt_v4i fa[4];
#pragma unroll
			for (int32_t m = 0; m < 4; ++m) fa[m] = *(const qt_v4i *)((const char *)sh_g + (wi + 16 * m + fr) * QT_LD + ks + fk);
#pragma unroll
			for (int32_t n = 0; n < 4; ++n) {
				const int32_t off = (wj + 16 * n + fr) * QT_LD + ks + fk;
				const qt_v4i fl = *(const qt_v4i *)((const char *)sh_lo + off);
#pragma unroll
				for (int32_t m = 0; m < 4; ++m) acc_lo[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m], fl, acc_lo[m][n], 0, 0, 0);
				if constexpr (HI) {
					const qt_v4i fh = *(const qt_v4i *)((const char *)sh_hi + off);
#pragma unroll
					for (int32_t m = 0; m < 4; ++m) acc_hi[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m], fh, acc_hi[m][n], 0, 0, 0);
				}
			}
		}
		__syncthreads();
	}

	// the epilogue: register r of tile (m, n) is gene i0 + wi + 16 m + 4 (lane >> 4) + r, permutation j0 + wj + 16 n + (lane & 15)
	uint32_t col_ok = 0;
#pragma unroll
	for (int32_t n = 0; n < 4; ++n) col_ok |= (uint32_t)(j0 + wj + 16 * n + fr < nb) << n;
#pragma unroll
	for (int32_t m = 0; m < 4; ++m)
#pragma unroll
		for (int32_t r = 0; r < 4; ++r) {
			const int32_t g = i0 + wi + 16 * m + 4 * (lane >> 4) + r;
			const int32_t thr = g < G ? absd[g] : QT_NEVER;
			int32_t hits = 0;
#pragma unroll
			for (int32_t n = 0; n < 4; ++n) {
				int32_t d = acc_lo[m][n][r];
				if constexpr (HI) d += 256 * acc_hi[m][n][r];
				const bool here = col_ok >> n & 1u;
				hits += (int32_t)(here && (d < 0 ? -d : d) >= thr);
				if (d_rows != nullptr && here && g < G) d_rows[(size_t)(j0 + wj + 16 * n + fr) * (size_t)G + (size_t)g] = d;
			}
			hits += __shfl_xor(hits, 1, WAVE);
			hits += __shfl_xor(hits, 2, WAVE);
			hits += __shfl_xor(hits, 4, WAVE);
			hits += __shfl_xor(hits, 8, WAVE);
			if (fr == 0 && hits > 0) atomicAdd(k_out + g, hits);
		}
}
