// ------------------------------------------------------------------------------------------------
// PERMANOVA (pga_pan_permanova; DESIGN.md section 8 "PERMANOVA"): do the two groups of one label row differ in a distance matrix as a
// whole.  With N columns, e = q >> s, w = e^2 (int64, zero diagonal), r[i] = sum_j w[i][j], T = sum r: a label row y gives
// A(y) = sum over ordered pairs of y_i y_j w[i][j], B(y) = sum y_i r[i] and G(y) = N A - 2 n1 B, which orders the within-group sum of
// squares; k counts the permutations p with G(y_p) <= G(y).  Over all permutations A_p = y_p . W . y_p is a matrix product followed by a
// masked row sum: the second kernel of this project on the matrix cores, after k_qtrait_count, whose staging and lane maps it keeps.
//   prep   k_perma_prep: one workgroup per row of the padded matrix.  w as D balanced base-256 signed-byte digit planes pl[D][Np][Np],
//          w = sum d_k 256^k with d_k in [-128, 127] by k_qtrait_perm's lo / hi rule repeated (d = ((w + 128) & 255) - 128,
//          w = (w - d) >> 8); Np = N rounded up to PM_TILE, rows and columns past N zero; D the smallest count that holds the largest
//          w (the host's: 127 (256^D - 1) / 255 >= max w, D <= 8 below 2^62).  Also r[i], and T by one 64-bit atomicAdd a row.
//   rows   k_trait_perm, unchanged: bit rows [nb][W] of one batch of permutations.
//   quad   k_perma_quad: an int8 GEMM on v_mfma_i32_16x16x64_i8.  One workgroup of four waves per 128 columns x 128 permutations x
//          plane, each wave 64 x 64 as 4 x 4 MFMA tiles.  The A operand is the permutation BIT rows, expanded to 0/1 bytes on their way
//          into LDS (qt_nibble_bytes); the B operand is the plane's rows j with K = i contiguous -- w is symmetric, so the row-major
//          plane is already K-major.  Rows are QT_LD = 144 bytes apart, operand and result maps as k_qtrait_count states them: result
//          row = 4 (lane >> 4) + register is the A side (permutation), column = lane & 15 the B side (matrix column).
//          Symmetry: for column tile J the K loop ends at J's own chunk, and the accumulators are doubled (acc += acc) before that
//          last, diagonal chunk is added: an ordered pair (i, j) with i in an earlier tile stands for (j, i) too, and the diagonal
//          block's full square already holds both orders.  Half the work.  |acc| <= 2 x 128 x N = 2^22 at N = 16 384: int32 holds it,
//          and the 64 columns a lane group sums stay below 2^28.
//          Epilogue: acc[p][j] masked by bit j of row p and summed over the tile's columns (the four tiles in the lane, then four
//          __shfl_xor over the 16 lanes that share a permutation), times 256^plane in uint64, ONE 64-bit atomicAdd per (wave tile,
//          permutation) into A[p].  A plane's partial sum may be negative or pass 2^63 on its own; unsigned adds wrap and commute, and
//          the true total over planes and tiles is below 2^62, so what stands in A[p] after the last add is that total whatever the
//          order of the adds: an overflowing partial sum is harmless and A does not depend on scheduling.
//   stat   k_perma_stat: 8 lanes per permutation walk the set bits of its row for B_p; G_p = N A_p - 2 n1 B_p in __int128 against
//          G of the observed row (out[1], out[2]: the observed row goes through quad and stat first, as a one-row batch, so both stand in
//          device memory before any count reads them), permutations past the batch masked, one atomicAdd per wave into k.  It clears
//          A[p] behind itself for the next batch.
// ------------------------------------------------------------------------------------------------
constexpr int32_t PM_TILE = QT_TILE;   // columns and permutations of a workgroup's tile; Np is a multiple of it
constexpr int32_t PM_ROW_LANES = 8;    // lanes that share one permutation in k_perma_stat
constexpr int32_t PM_MAX_PLANE = 8;
enum { PM_T = 0, PM_A = 1, PM_B = 2, PM_K = 3, PM_N_OUT = 4 }; // out[]: T, A and B of the observed row, k

// grid: Np workgroups.  q[N][N]; pl[D][Np][Np]; r[N]; out[PM_T] += the row's sum
__global__ __launch_bounds__(BLOCK) void k_perma_prep(const int32_t *__restrict__ q, int32_t N, int32_t Np, int32_t shift, int32_t D, int8_t *__restrict__ pl,
                                                      long long *__restrict__ r, unsigned long long *__restrict__ out)
{
	__shared__ unsigned long long part[BLOCK / WAVE];
	const int32_t i = (int32_t)blockIdx.x, t = (int32_t)threadIdx.x;
	const size_t plane = (size_t)Np * (size_t)Np;
	unsigned long long sum = 0;
	for (int32_t c = 4 * t; c < Np; c += 4 * BLOCK) { // four columns a lane: one 32-bit store per plane (Np is a multiple of 4)
		long long w[4];
#pragma unroll
		for (int32_t e = 0; e < 4; ++e) {
			const int32_t j = c + e;
			const long long v = i < N && j < N && j != i ? (long long)(q[(size_t)i * (size_t)N + (size_t)j] >> shift) : 0;
			w[e] = v * v, sum += (unsigned long long)w[e];
		}
		uint32_t *dst = (uint32_t *)(pl + (size_t)i * (size_t)Np + (size_t)c);
		for (int32_t k = 0; k < D; ++k) {
			uint32_t word = 0;
#pragma unroll
			for (int32_t e = 0; e < 4; ++e) {
				const long long d = ((w[e] + 128) & 255) - 128;
				w[e] = (w[e] - d) >> 8;
				word |= (uint32_t)(d & 255) << (8 * e);
			}
			dst[(size_t)k * (plane / 4)] = word;
		}
	}
	sum = wave_sum64(sum);
	if ((t & (WAVE - 1)) == 0) part[t / WAVE] = sum;
	__syncthreads();
	if (t == 0 && i < N) {
		unsigned long long row = 0;
#pragma unroll
		for (int32_t k = 0; k < BLOCK / WAVE; ++k) row += part[k];
		r[i] = (long long)row;
		atomicAdd(out + PM_T, row);
	}
}

// grid: (Np / 128, ceil(nb / 128), D).  rows[nb][W] with the bits past N zero, pl[D][Np][Np]; a_out[p] += the share of the column tile
// and the plane in A of permutation p of the batch
__global__ __launch_bounds__(BLOCK, 2) void k_perma_quad(const uint32_t *__restrict__ rows, const int8_t *__restrict__ pl, int32_t nb, int32_t W, int32_t Np,
                                                         unsigned long long *__restrict__ a_out)
{
	__shared__ uint4 sh_y[PM_TILE * QT_LD / 16], sh_w[PM_TILE * QT_LD / 16];
	const int32_t t = (int32_t)threadIdx.x, lane = t & (WAVE - 1), wv = t / WAVE;
	const int32_t j0 = (int32_t)blockIdx.x * PM_TILE, p0 = (int32_t)blockIdx.y * PM_TILE, plane = (int32_t)blockIdx.z;
	const int8_t *w = pl + (size_t)plane * (size_t)Np * (size_t)Np;
	const int32_t wi = (wv >> 1) * 64, wj = (wv & 1) * 64; // the wave's 64 x 64 corner in the tile: permutations, columns
	const int32_t fr = lane & 15, fk = (lane >> 4) * 16;   // operand fragment: row / column, first byte of the step

	qt_v4i acc[4][4];
#pragma unroll
	for (int32_t m = 0; m < 4; ++m)
#pragma unroll
		for (int32_t n = 0; n < 4; ++n) acc[m][n] = qt_v4i{0, 0, 0, 0};

	// staging: thread t expands words 2 (t & 1), + 1 of permutation row t >> 1 (64 columns) and copies 16 bytes x 4 of the plane
	const int32_t sy_row = t >> 1, sy_half = t & 1;
	const bool sy_ok = p0 + sy_row < nb; // rows past the batch: zero (and never added in the epilogue)
	const uint32_t *sy_src = rows + (size_t)(sy_ok ? p0 + sy_row : 0) * (size_t)W;
	for (int32_t k0 = 0; k0 <= j0; k0 += QT_KC) {
		{
			const int32_t w0 = (k0 >> 5) + 2 * sy_half;
			const uint32_t b0 = sy_ok && w0 < W ? sy_src[w0] : 0u, b1 = sy_ok && w0 + 1 < W ? sy_src[w0 + 1] : 0u;
			uint4 *dst = sh_y + (sy_row * QT_LD + sy_half * 64) / 16;
#pragma unroll
			for (int32_t q = 0; q < 2; ++q) {
				const uint32_t b = q ? b1 : b0;
				dst[2 * q] = make_uint4(qt_nibble_bytes(b), qt_nibble_bytes(b >> 4), qt_nibble_bytes(b >> 8), qt_nibble_bytes(b >> 12));
				dst[2 * q + 1] = make_uint4(qt_nibble_bytes(b >> 16), qt_nibble_bytes(b >> 20), qt_nibble_bytes(b >> 24), qt_nibble_bytes(b >> 28));
			}
		}
#pragma unroll
		for (int32_t q = 0; q < 4; ++q) { // (j0 + row < Np and k0 + 127 < Np: the planes are padded to whole tiles)
			const int32_t idx = t + BLOCK * q, row = idx >> 3, seg = idx & 7;
			sh_w[(row * QT_LD + seg * 16) / 16] = *(const uint4 *)(w + (size_t)(j0 + row) * (size_t)Np + (size_t)(k0 + seg * 16));
		}
		__syncthreads();
		if (k0 == j0) { // the diagonal chunk is next: what stands so far counts for both orders of its pairs
#pragma unroll
			for (int32_t m = 0; m < 4; ++m)
#pragma unroll
				for (int32_t n = 0; n < 4; ++n) acc[m][n] += acc[m][n];
		}
#pragma unroll
		for (int32_t ks = 0; ks < QT_KC; ks += 64) {
			qt_v4i fa[4];
#pragma unroll
			for (int32_t m = 0; m < 4; ++m) fa[m] = *(const qt_v4i *)((const char *)sh_y + (wi + 16 * m + fr) * QT_LD + ks + fk);
#pragma unroll
			for (int32_t n = 0; n < 4; ++n) {
				const qt_v4i fb = *(const qt_v4i *)((const char *)sh_w + (wj + 16 * n + fr) * QT_LD + ks + fk);
#pragma unroll
				for (int32_t m = 0; m < 4; ++m) acc[m][n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[m], fb, acc[m][n], 0, 0, 0);
			}
		}
		__syncthreads();
	}

	// the epilogue: register r of tile (m, n) is permutation p0 + wi + 16 m + 4 (lane >> 4) + r, column j0 + wj + 16 n + (lane & 15);
	// the wave's 64 columns are the two words (j0 + wj) / 32, + 1 of the permutation's row
	const int32_t wd = (j0 + wj) >> 5;
#pragma unroll
	for (int32_t m = 0; m < 4; ++m)
#pragma unroll
		for (int32_t r = 0; r < 4; ++r) {
			const int32_t p = p0 + wi + 16 * m + 4 * (lane >> 4) + r;
			const bool p_ok = p < nb;
			const uint32_t *row = rows + (size_t)(p_ok ? p : 0) * (size_t)W;
			const uint32_t y0 = p_ok && wd < W ? row[wd] : 0u, y1 = p_ok && wd + 1 < W ? row[wd + 1] : 0u;
			int32_t sum = 0;
#pragma unroll
			for (int32_t n = 0; n < 4; ++n) sum += ((n < 2 ? y0 : y1) >> (16 * (n & 1) + fr) & 1u) ? acc[m][n][r] : 0;
			sum += __shfl_xor(sum, 1, WAVE);
			sum += __shfl_xor(sum, 2, WAVE);
			sum += __shfl_xor(sum, 4, WAVE);
			sum += __shfl_xor(sum, 8, WAVE);
			// unsigned: the adds wrap and commute, the total is below 2^62 (see the head of this file)
			if (fr == 0 && p_ok && sum != 0) atomicAdd(a_out + p, (unsigned long long)(long long)sum << (8 * plane));
		}
}

__device__ __forceinline__ long long row8_sum64(long long v)
{
	v += __shfl_xor(v, 1, WAVE);
	v += __shfl_xor(v, 2, WAVE);
	return v + __shfl_xor(v, 4, WAVE);
}

// grid: ceil(nb / 32).  observed: the batch is the observed row alone, out[PM_A] and out[PM_B] are written; otherwise
// out[PM_K] += #{p < nb : G_p <= G of those}.  a[p] is read and cleared.  a_rows / b_rows: NULL, or (tests) A_p and B_p of the batch
__global__ __launch_bounds__(BLOCK) void k_perma_stat(const uint32_t *__restrict__ rows, const long long *__restrict__ r, int32_t nb, int32_t W, int32_t N, int32_t n1,
                                                      bool observed, unsigned long long *__restrict__ a, long long *__restrict__ out,
                                                      long long *__restrict__ a_rows, long long *__restrict__ b_rows)
{
	const int64_t p = (int64_t)blockIdx.x * (BLOCK / PM_ROW_LANES) + (int64_t)(threadIdx.x / PM_ROW_LANES);
	const int32_t l = (int32_t)threadIdx.x % PM_ROW_LANES;
	long long b = 0;
	if (p < nb) {
		const uint32_t *row = rows + (size_t)p * (size_t)W;
		for (int32_t k = l; k < W; k += PM_ROW_LANES)
			for (uint32_t x = row[k]; x; x &= x - 1) b += r[k * 32 + __ffs((int32_t)x) - 1]; // (bits past N are zero)
	}
	b = row8_sum64(b);
	bool hit = false;
	if (p < nb && l == 0) {
		const long long ap = (long long)a[p];
		a[p] = 0;
		if (a_rows != nullptr) a_rows[p] = ap;
		if (b_rows != nullptr) b_rows[p] = b;
		if (observed) out[PM_A] = ap, out[PM_B] = b;
		else {
			const __int128 g = (__int128)N * ap - (__int128)(2 * (long long)n1) * b;
			const __int128 g_obs = (__int128)N * out[PM_A] - (__int128)(2 * (long long)n1) * out[PM_B];
			hit = g <= g_obs;
		}
	}
	const unsigned long long hits = __ballot(hit);
	if ((threadIdx.x & (WAVE - 1)) == 0 && hits != 0) atomicAdd((unsigned long long *)(out + PM_K), (unsigned long long)__popcll(hits));
}
