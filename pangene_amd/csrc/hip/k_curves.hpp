// ------------------------------------------------------------------------------------------------
// Pangenome accumulation curves (pga_pan_curves): pan, core, new and unique genes as the columns of a presence matrix are added in
// n orders.  Per (order p, gene g) three ranks in the order: f1 = the first column where g is present, f2 = the second, z = the first
// where it is absent (n_asm when there is none).  Over the first k columns g is in the pan genome iff f1 < k, new at k iff f1 = k - 1,
// unique iff f1 < k <= f2 and core iff z >= k, so the curves are prefix sums of three histograms per order.
// A rank is found either from the gene's list of present (absent) columns -- the least rank over the list -- or by walking the order
// from rank 0 and testing the gene's bit row, whichever is cheaper: a gene with c present columns keeps a list when min(c, A - c) is at
// most T ~ sqrt(2A), and a walk for the other side ends after about A / c (A / (A - c)) steps, so no (order, gene) costs more than
// O(sqrt(A)) expected, and core and cloud genes almost nothing.
//   k_curves_rank    rank[p][order[p][i]] = i
//   k_curves_count   per gene: present columns, list length            -> scan -> list offsets
//   k_curves_fill    per gene: its list (present or absent columns, ascending)
//   k_curves_ranks   per (order, gene): f1, f2, z into per-order histograms of A + 1 bins each; the bins below R and the sentinel A in
//                    LDS (R = A when 3 (A + 1) counters fit the share), the others straight to the global histograms
//   k_curves_finish  per order: the three prefix sums and the four curves
// ------------------------------------------------------------------------------------------------

constexpr int32_t CURVES_LDS_BINS = 4096; // LDS bins per histogram (3 x 4 096 x 4 B = 48 KiB): ranks 0 .. 4 094 and the sentinel

// which list a gene keeps: 1 its present columns, 2 its absent columns, 0 none (both sides are walked)
__device__ __forceinline__ int curves_kind(int32_t c, int32_t A, int32_t T)
{
	if (c <= A - c) return c <= T ? 1 : 0;
	return A - c <= T ? 2 : 0;
}
__device__ __forceinline__ uint32_t curves_word(const uint32_t *row, int32_t w, int32_t W, int32_t A)
{
	uint32_t x = row[w];
	if (w == W - 1 && (A & 31)) x &= (1u << (A & 31)) - 1u; // bits past the last column do not count
	return x;
}

__global__ __launch_bounds__(BLOCK) void k_curves_rank(const int32_t *ord, int64_t n_tot, int32_t A, int32_t *rank)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n_tot) return;
	const int64_t p = i / A;
	rank[p * A + ord[i]] = (int32_t)(i - p * A);
}

__global__ __launch_bounds__(BLOCK) void k_curves_count(const uint32_t *bits, int32_t W, int32_t G, int32_t A, int32_t T, int32_t *cnt, int32_t *len)
{
	const int32_t g = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	if (g >= G) return;
	const uint32_t *row = bits + (size_t)g * W;
	int32_t c = 0;
	for (int32_t w = 0; w < W; ++w) c += __popc(curves_word(row, w, W, A));
	const int k = curves_kind(c, A, T);
	cnt[g] = c, len[g] = k == 1 ? c : k == 2 ? A - c : 0;
}

__global__ __launch_bounds__(BLOCK) void k_curves_fill(const uint32_t *bits, int32_t W, int32_t G, int32_t A, int32_t T, const int32_t *cnt,
                                                       const int32_t *off, int32_t *list)
{
	const int32_t g = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	if (g >= G) return;
	const int k = curves_kind(cnt[g], A, T);
	if (k == 0) return;
	const uint32_t *row = bits + (size_t)g * W;
	int32_t *o = list + off[g];
	for (int32_t w = 0; w < W; ++w) {
		uint32_t x = curves_word(row, w, W, A);
		if (k == 2) x = ~x & (w == W - 1 && (A & 31) ? (1u << (A & 31)) - 1u : 0xffffffffu);
		while (x) { *o++ = w * 32 + __ffs(x) - 1; x &= x - 1; }
	}
}

// grid: n_perm * bpo blocks, block b of order p takes genes b * BLOCK + t, + bpo * BLOCK, ...; LDS: 3 * (R + 1) counters
__global__ __launch_bounds__(BLOCK) void k_curves_ranks(const uint32_t *bits, int32_t W, const int32_t *ord, const int32_t *rank,
                                                        const int32_t *cnt, const int32_t *off, const int32_t *list, int32_t G, int32_t A,
                                                        int32_t T, int32_t R, int32_t bpo, int32_t *hist)
{
	extern __shared__ int32_t sh_hist[];
	const int32_t p = (int32_t)(blockIdx.x / bpo), b = (int32_t)(blockIdx.x % bpo);
	const int32_t nb = 3 * (R + 1);
	for (int32_t i = threadIdx.x; i < nb; i += BLOCK) sh_hist[i] = 0;
	__syncthreads();
	const int32_t *o = ord + (size_t)p * A, *rk = rank + (size_t)p * A;
	int32_t *h = hist + (size_t)p * 3 * (A + 1);
	auto add = [&](int s, int32_t v) {
		if (v == A) atomicAdd(&sh_hist[s * (R + 1) + R], 1);
		else if (v < R) atomicAdd(&sh_hist[s * (R + 1) + v], 1);
		else atomicAdd(&h[(size_t)s * (A + 1) + v], 1);
	};
	for (int32_t g = b * BLOCK + (int32_t)threadIdx.x; g < G; g += bpo * BLOCK) {
		const int32_t c = cnt[g];
		const int k = curves_kind(c, A, T);
		const uint32_t *row = bits + (size_t)g * W;
		const int32_t *lst = list + off[g];
		int32_t f1 = A, f2 = A, z = A;
		if (k == 1) {
			for (int32_t i = 0; i < c; ++i) {
				const int32_t r = rk[lst[i]];
				if (r < f1) f2 = f1, f1 = r;
				else if (r < f2) f2 = r;
			}
		} else if (c > 0) {
			for (int32_t r = 0; r < A; ++r) {
				const int32_t j = o[r];
				if ((row[j >> 5] >> (j & 31)) & 1u) { if (f1 == A) f1 = r; else { f2 = r; break; } }
			}
		}
		if (k == 2) {
			for (int32_t i = 0; i < A - c; ++i) z = min(z, rk[lst[i]]);
		} else if (c < A) {
			for (int32_t r = 0; r < A; ++r) {
				const int32_t j = o[r];
				if (!((row[j >> 5] >> (j & 31)) & 1u)) { z = r; break; }
			}
		}
		add(0, f1), add(1, f2), add(2, z);
	}
	__syncthreads();
	for (int32_t i = threadIdx.x; i < nb; i += BLOCK) {
		const int32_t v = sh_hist[i];
		if (v == 0) continue;
		const int32_t s = i / (R + 1), bin = i - s * (R + 1);
		atomicAdd(&h[(size_t)s * (A + 1) + (bin == R ? A : bin)], v);
	}
}

// one block per order: inclusive prefix sums c1, c2, cz of the three histograms; at column k = i + 1: pan = c1[i], core = G - cz[i],
// new = h1[i], unique = c1[i] - c2[i].  out[4][n_perm][A]
__global__ __launch_bounds__(BLOCK) void k_curves_finish(const int32_t *hist, int32_t A, int32_t G, int32_t n_perm, int32_t *out)
{
	__shared__ int32_t part[3][BLOCK];
	const int32_t p = (int32_t)blockIdx.x, t = (int32_t)threadIdx.x;
	const int32_t *h1 = hist + (size_t)p * 3 * (A + 1), *h2 = h1 + (A + 1), *hz = h2 + (A + 1);
	const int32_t chunk = (A + BLOCK - 1) / BLOCK, lo = min(A, t * chunk), hi = min(A, lo + chunk);
	int32_t s1 = 0, s2 = 0, sz = 0;
	for (int32_t i = lo; i < hi; ++i) s1 += h1[i], s2 += h2[i], sz += hz[i];
	part[0][t] = s1, part[1][t] = s2, part[2][t] = sz;
	__syncthreads();
	if (t < 3) { // exclusive scan of the BLOCK partial sums, one histogram per thread
		int32_t run = 0;
		for (int32_t k = 0; k < BLOCK; ++k) { const int32_t v = part[t][k]; part[t][k] = run; run += v; }
	}
	__syncthreads();
	int32_t c1 = part[0][t], c2 = part[1][t], cz = part[2][t];
	const size_t plane = (size_t)n_perm * A, base = (size_t)p * A;
	for (int32_t i = lo; i < hi; ++i) {
		c1 += h1[i], c2 += h2[i], cz += hz[i];
		out[base + i] = c1;
		out[plane + base + i] = G - cz;
		out[2 * plane + base + i] = h1[i];
		out[3 * plane + base + i] = c1 - c2;
	}
}
