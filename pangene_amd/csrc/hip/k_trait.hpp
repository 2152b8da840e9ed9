// ------------------------------------------------------------------------------------------------
// Gene-trait association (pga_pan_trait): the third member of the k_dist.hpp / k_assoc.hpp family -- an all-pairs AND + popcount over
// bit rows, here GENE rows against PERMUTED COPIES OF ONE LABEL ROW.  With N columns, y the label row, t = |y|, a = |B_g|,
// s = |B_g & y|, D = s N - a t: permutation p gives s_p = |B_g & y_p|, D_p = s_p N - a t, and k_g counts the p with |D_p| >= |D|.
// For fixed a, t, N that is s_p <= lo_g or s_p >= hi_g with lo_g = floor((a t - |D|) / N) and hi_g = ceil((a t + |D|) / N).
//   obs    k_trait_obs: a, s of every row (8 lanes a row, as k_assoc_count), the two thresholds and the eligibility; a row that is not
//          eligible gets lo = -1 and hi = INT32_MAX, which no count meets.
//   perm   k_trait_perm: the label rows of one batch of permutations, made here from the one uploaded label row.  One lane per
//          permutation runs the pinned swap sequence (k_perm.hpp) over a private bit row: swapping the bits i and j of the row is what
//          applying the order to the labels gives.  The wave's 64 rows are laid out as k_perm.hpp says, in LDS while they fit
//          (W <= 128, N <= 4 096) and in a global scratch buffer beyond; the finished rows are written row-major for the count kernel.
//   count  k_trait_count: one workgroup per 128 genes x 128 permutations, the tile body of k_dist_shared / k_assoc_pairs (BIT_TILE,
//          k_dist.hpp) with the inner loop trimmed to the rows' last word.  Rectangular grid (x: gene tile, y: permutation tile of the
//          batch).  Epilogue: each count against its row's lo / hi, the hits of a row summed over the 16 lanes that share it, ONE
//          atomicAdd per (tile, row) with a hit into k[g].
// ------------------------------------------------------------------------------------------------
constexpr int32_t TRAIT_ROW_LANES = 8;     // lanes that share one row in k_trait_obs (row8_sum)
constexpr int32_t TRAIT_PERM_LDS_W = 128;  // words of a label row up to which a wave's 64 rows stay in LDS (32 KiB)
constexpr int32_t TRAIT_NEVER_LO = -1, TRAIT_NEVER_HI = 0x7fffffff;

__global__ __launch_bounds__(BLOCK) void k_trait_obs(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ label, int32_t G, int32_t W, int32_t N,
                                                     int32_t t_sum, int32_t min_count, int32_t *__restrict__ a_out, int32_t *__restrict__ s_out,
                                                     int32_t *__restrict__ lo_out, int32_t *__restrict__ hi_out)
{
	const int64_t g = (int64_t)blockIdx.x * (BLOCK / TRAIT_ROW_LANES) + (int64_t)(threadIdx.x / TRAIT_ROW_LANES);
	const int32_t l = (int32_t)threadIdx.x % TRAIT_ROW_LANES;
	int32_t a = 0, s = 0;
	if (g < G) {
		const uint32_t *row = bits + (size_t)g * (size_t)W;
		for (int32_t k = l; k < W; k += TRAIT_ROW_LANES) {
			const uint32_t w = row[k];
			a += __popc(w), s += __popc(w & label[k]);
		}
	}
	a = row8_sum(a), s = row8_sum(s);
	if (g < G && l == 0) {
		int32_t lo = TRAIT_NEVER_LO, hi = TRAIT_NEVER_HI;
		if (min(a, N - a) >= min_count) {
			const int64_t c = (int64_t)a * t_sum, d0 = (int64_t)s * N - c, d = d0 < 0 ? -d0 : d0; // all below 2^48
			lo = c >= d ? (int32_t)((c - d) / N) : -1;
			hi = (int32_t)((c + d + N - 1) / N);
		}
		a_out[g] = a, s_out[g] = s, lo_out[g] = lo, hi_out[g] = hi;
	}
}

// perm_wave_rows (k_perm.hpp) over rows of W words: permutation p0 + q of the batch is row q of rows[nb][W].  USE_LDS: the wave's rows
// in LDS; otherwise in work[workgroup][W][64].
template <bool USE_LDS>
__global__ __launch_bounds__(WAVE) void k_trait_perm(const uint32_t *__restrict__ label, int32_t N, int32_t W, uint32_t seed, uint32_t p0, int32_t nb,
                                                     uint32_t *__restrict__ work, uint32_t *__restrict__ rows)
{
	perm_wave_rows<uint32_t, TRAIT_PERM_LDS_W, USE_LDS>(
		W, N, seed, p0, nb, work, [&](int32_t k) { return label[k]; },
		[](uint32_t *row, int32_t i, int32_t j) {
			const int32_t wi = (i >> 5) * WAVE, wj = (j >> 5) * WAVE;
			const uint32_t d = ((row[wi] >> (i & 31)) ^ (row[wj] >> (j & 31))) & 1u; // the two labels differ: both flip
			row[wi] ^= d << (i & 31);
			row[wj] ^= d << (j & 31); // (read again: wi may be wj)
		},
		[&](const uint32_t *fin, int64_t q, int32_t l) { perm_row_major(fin, rows + (size_t)q * (size_t)W, W, l); });
}

// grid: (ceil(G / 128), ceil(nb / 128)).  bits[G][W], rows[nb][W], lo / hi[G]; k[g] += hits
__global__ __launch_bounds__(BLOCK, 2) void k_trait_count(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ rows, const int32_t *__restrict__ lo,
                                                         const int32_t *__restrict__ hi, int32_t G, int32_t nb, int32_t W, int32_t n_chunk,
                                                         int32_t *__restrict__ k_out)
{
	__shared__ uint4 sh4[DIST_LDS_WORDS / 4];
	uint32_t *sh = (uint32_t *)sh4;
	const int32_t t = (int32_t)threadIdx.x, tx = t & 15, ty = t >> 4;
	const int32_t i0 = (int32_t)blockIdx.x * DIST_TILE, j0 = (int32_t)blockIdx.y * DIST_TILE;

	BIT_TILE(true, bits, G, rows, nb, W, 0, n_chunk)

	// the epilogue: the thread's 8 columns that exist, then per row its 8 counts against the row's thresholds; the 16 lanes tx = 0..15
	// of a row are neighbours in the wave, so four shuffles sum the row's hits and lane tx = 0 adds them
	uint32_t col_ok = 0;
#pragma unroll
	for (int32_t jj = 0; jj < 8; ++jj) col_ok |= (uint32_t)(j0 + tx + 16 * jj < nb) << jj;
#pragma unroll
	for (int32_t ii = 0; ii < 8; ++ii) {
		const int32_t g = i0 + ty + 16 * ii;
		const int32_t l = g < G ? lo[g] : TRAIT_NEVER_LO, h = g < G ? hi[g] : TRAIT_NEVER_HI;
		int32_t hits = 0;
#pragma unroll
		for (int32_t jj = 0; jj < 8; ++jj) {
			const int32_t s = (int32_t)acc[ii][jj];
			hits += (int32_t)((col_ok >> jj & 1u) && (s <= l || s >= h));
		}
		hits += __shfl_xor(hits, 1, WAVE);
		hits += __shfl_xor(hits, 2, WAVE);
		hits += __shfl_xor(hits, 4, WAVE);
		hits += __shfl_xor(hits, 8, WAVE);
		if (tx == 0 && hits > 0) atomicAdd(k_out + g, hits);
	}
}
