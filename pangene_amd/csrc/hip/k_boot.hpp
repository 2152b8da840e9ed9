// k_boot.hpp -- the bootstrap of pangene tree (pga_pan_boot, include/pangene_hip.h; DESIGN.md section 8 "Bootstrap"): replicate b draws
// n_item items with replacement, and its tree is the tree of the resampled bit rows.  Included by pga_backend.hip behind k_dist.hpp and
// k_join.hpp; uses BLOCK / WAVE from there.  Everything stays on the device from the bit rows to the records:
//   draws     k_boot_draw: m_t of (replicate, t), one thread a draw -- counter-based (draw t needs no earlier draw), so the 64-bit
//             modulo is paid once per draw here and not once per assembly.
//   rows      k_boot_resample: destination word w of (replicate, assembly a) holds bits t = 32 w .. 32 w + 31, each = bit m_t of row a.
//             A thread owns one destination word: it reads its 32 draws once, keeps them in registers and reuses them over the
//             assemblies of its workgroup, whose source rows pass through LDS one after the other (up to 64 KiB: n_item <= 524 288);
//             consecutive threads write consecutive words.  A longer row is read where it is (USE_LDS = false).
//   counts    S_b by k_dist_shared, one launch a replicate.
//   distances k_boot_maxdiff (diff only: the largest difference of a replicate, which sets its F) and k_boot_fixed: S_b -> q_b in
//             d[.][ld], both formulas in 64-bit integers exactly as tree.cpp's to_fixed.
//   joins     the batched twins of k_join.hpp.
#pragma once

constexpr int32_t BOOT_LDS_WORDS = 16384; // the source row's window in LDS: 64 KiB

// grid: (ceil(M / BLOCK), n_rep); replicate first + blockIdx.y -> draws[blockIdx.y][M].  M >= 1.
__global__ __launch_bounds__(BLOCK) void k_boot_draw(int32_t M, uint32_t seed, uint32_t first, int32_t *__restrict__ draws)
{
	const int64_t t = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (t >= M) return;
	const uint64_t x0 = mix64((uint64_t)seed << 32 | (uint64_t)(first + blockIdx.y));
	draws[(size_t)blockIdx.y * (size_t)M + (size_t)t] = (int32_t)(mix64(x0 + (uint64_t)(t + 1) * 0x9E3779B97F4A7C15ull) % (uint64_t)M);
}

// grid: (ceil(W / BLOCK), ceil(A / a_per), n_rep); bits[A][W] -> rows[blockIdx.z][A][W].  Dynamic LDS: W words when USE_LDS.
template <bool USE_LDS>
__global__ __launch_bounds__(BLOCK) void k_boot_resample(const uint32_t *__restrict__ bits, const int32_t *__restrict__ draws, int32_t M, int32_t W, int32_t A,
                                                         int32_t a_per, uint32_t *__restrict__ rows)
{
	extern __shared__ uint32_t boot_row[];
	const int32_t w = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	const int32_t a0 = (int32_t)blockIdx.y * a_per, a1 = min(A, a0 + a_per);
	const size_t q = blockIdx.z;
	int32_t m[32]; // this word's draws; -1 past M: the bit stays zero
#pragma unroll
	for (int k = 0; k < 32; ++k) {
		const int64_t t = (int64_t)w * 32 + k;
		m[k] = (w < W && t < M) ? draws[q * (size_t)M + (size_t)t] : -1;
	}
	for (int32_t a = a0; a < a1; ++a) {
		const uint32_t *src = bits + (size_t)a * (size_t)W;
		if (USE_LDS) {
			__syncthreads(); // everyone is done with the previous row
			for (int32_t i = (int32_t)threadIdx.x; i < W; i += BLOCK) boot_row[i] = src[i];
			__syncthreads();
		}
		if (w >= W) continue;
		const uint32_t *from = USE_LDS ? boot_row : src;
		uint32_t v = 0;
#pragma unroll
		for (int k = 0; k < 32; ++k)
			if (m[k] >= 0) v |= (from[m[k] >> 5] >> (m[k] & 31) & 1u) << k;
		rows[(q * (size_t)A + (size_t)a) * (size_t)W + (size_t)w] = v;
	}
}

// grid: (x, n_rep), x workgroups striding over the A * A entries of S[blockIdx.y]: mx[blockIdx.y] = max(n_i + n_j - 2 s) (the host zeroed it;
// a difference is a count of items, so it is not negative and fits 31 bits)
__global__ __launch_bounds__(BLOCK) void k_boot_maxdiff(const int32_t *__restrict__ S, int32_t A, int32_t *__restrict__ mx)
{
	const size_t nn = (size_t)A * (size_t)A;
	const int32_t *s = S + (size_t)blockIdx.y * nn;
	int32_t best = 0;
	for (size_t e = (size_t)blockIdx.x * BLOCK + threadIdx.x; e < nn; e += (size_t)gridDim.x * BLOCK) {
		const size_t i = e / (size_t)A, j = e - i * (size_t)A;
		best = max(best, (int32_t)((long long)s[i * A + i] + s[j * A + j] - 2 * (long long)s[e]));
	}
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1) best = max(best, __shfl_xor(best, o, WAVE));
	if (threadIdx.x % WAVE == 0 && best > 0) atomicMax(&mx[blockIdx.y], best);
}

// grid: (A, n_rep), one workgroup per row: S[blockIdx.y][A][A] -> d[blockIdx.y][A][ld], the columns past A zero.  diff: F from mx, and
// F < 0 raises the replicate's flag.
__global__ __launch_bounds__(BLOCK) void k_boot_fixed(const int32_t *__restrict__ S, int32_t A, int32_t ld, int32_t diff, const int32_t *__restrict__ mx,
                                                      int32_t *__restrict__ d, int32_t *__restrict__ flag)
{
	const size_t q = blockIdx.y, i = blockIdx.x;
	const int32_t *s = S + q * (size_t)A * (size_t)A;
	int32_t *out = d + (q * (size_t)A + i) * (size_t)ld;
	int32_t F = 20;
	if (diff) {
		const int32_t bl = 32 - __clz(mx[q]); // (__clz(0) = 32)
		F = min(20, 29 - bl);
		if (F < 0) { if (threadIdx.x == 0 && i == 0) flag[q] = 1; F = 0; }
	}
	const long long ni = s[i * A + i];
	for (int32_t c = (int32_t)threadIdx.x; c < ld; c += BLOCK) {
		long long v = 0;
		if (c < A && (size_t)c != i) {
			const long long nj = s[(size_t)c * A + c], x = s[i * A + c];
			if (diff) v = (ni + nj - 2 * x) << F;
			else {
				const long long u = ni + nj - x;
				v = u == 0 ? 0 : ((1ll << 21) * (u - x) + u) / (2 * u);
			}
		}
		out[c] = (int32_t)v;
	}
}
