// k_medoids.hpp -- k-medoids (PAM) over a fixed-point distance matrix (pga_pan_medoids, include/pangene_hip.h; DESIGN.md section 8
// "Clusters").  Included by pga_backend.hip behind k_join.hpp; uses BLOCK / WAVE and join_block_min from there.
//
// State on the device: the matrix q[n][ld], the medoids med[slot] (assembly index, in the order they were picked; a swap puts the
// newcomer into the slot that retires), is_med[x] (slot or -1), and per column o its distance D[o] to the nearest medoid, DS[o] to the
// nearest of the others, and NN[o], the nearest one's slot (uint16: k <= 1 024).
//
// BUILD is two launches a step: k_med_gain (one workgroup per candidate row x, lanes on the columns, gain[x] = sum of max(0, D - q[x][.]),
// -1 for a medoid) and k_med_build_pick (one workgroup: largest gain, smallest x; the record; D = min(D, q[x][.])).  k_med_assign then
// gives D, DS and NN of every column from the k medoid rows and adds up removal[] and the cluster counts.
//
// SWAP never evaluates a clustering.  With d = q[x][o], taking medoid m out and x in changes column o by
//     min(d - D, 0)                        when NN[o] != m,
//     min(d, DS) - D                       when NN[o] == m,
// and the second line is the first plus (DS - D) + (d < D ? D - DS : min(d - DS, 0)).  So with
//     removal[m] = sum over {o : NN[o] = m} of DS[o] - D[o],
//     plus[x]    = sum over o of min(d - D[o], 0),
//     acc[m][x]  = sum over {o : NN[o] = m} of (d < D[o] ? D[o] - DS[o] : min(d - DS[o], 0)),
// delta(x, m) = TD(M - m + x) - TD(M) = removal[m] + acc[m][x] + plus[x], exactly.  Where a column is as near to a second medoid as to
// its nearest (D == DS) either of them may be NN[o]: taking either out leaves the column's distance at D, and both lines above then give
// min(d - D, 0).  So the sum does not depend on which way such ties fall, only on DS being the minimum over the medoids other than NN[o].
//
// One iteration: k_med_swap walks the matrix once -- the columns are counting-sorted by NN (perm), the matrix is symmetric, so the
// kernel walks ROWS perm[i] with the lanes on the candidates x: every load is a coalesced piece of a row, D / DS / NN of the row are the
// same in every lane, and a lane keeps its two int64 partial sums in registers.  The grid is (tiles of BLOCK candidates) x (chunks of the
// permuted row order); a chunk that crosses a cluster boundary flushes on the change of NN, and partial sums reach acc and plus by 64-bit
// atomicAdd (integer adds commute: the result does not depend on scheduling).  k_med_best takes, per candidate, the smallest
// (delta, medoid) and clears acc and plus behind itself; k_med_pick (one workgroup) takes the smallest (delta, x), raises `done` when it
// is not negative and swaps otherwise; k_med_assign and k_med_scatter rebuild D, DS, NN, removal and perm.  Every kernel of an iteration
// returns at once when `done` is set, so the host queues iterations in chunks and reads the status once a chunk.
//
// The finish reuses the row walk with f = d: labels by the medoid rule, perm by label, sums[c][o] = the sum of q[o][p] over the p of
// cluster c, transposed into the result.
#pragma once

constexpr int32_t MED_LIMIT = 1 << 29; // every entry is below this
constexpr int MED_MAX_K = 1024;
constexpr int MED_BATCH = 8;           // rows whose loads a lane has in flight
constexpr int MED_MIN_ROWS = 16;       // rows of a chunk at the least (without the override)
constexpr int MED_WANT_WG = 2048;      // workgroups the swap kernel aims for: eight per CU

struct MedStat { int32_t done, n_swap; };

__device__ __forceinline__ long long med_block_sum(long long s, unsigned long long *sh)
{
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);
	if (threadIdx.x % WAVE == 0) sh[threadIdx.x / WAVE] = (unsigned long long)s;
	__syncthreads();
	unsigned long long t = 0;
#pragma unroll
	for (int x = 0; x < BLOCK / WAVE; ++x) t += sh[x];
	return (long long)t;
}

// gain[x] of BUILD; one workgroup per row
__global__ __launch_bounds__(BLOCK) void k_med_gain(const int32_t *__restrict__ q, int32_t n, int32_t ld, const int32_t *__restrict__ D, const int32_t *__restrict__ is_med,
                                                    long long *__restrict__ gain)
{
	__shared__ unsigned long long sh[BLOCK / WAVE];
	const int32_t x = (int32_t)blockIdx.x;
	if (is_med[x] >= 0) { if (threadIdx.x == 0) gain[x] = -1; return; }
	const int32_t *row = q + (size_t)x * (size_t)ld;
	long long s = 0;
	for (int32_t o = (int32_t)threadIdx.x; o < n; o += BLOCK) {
		const int32_t v = D[o] - row[o];
		s += v > 0 ? v : 0;
	}
	s = med_block_sum(s, sh);
	if (threadIdx.x == 0) gain[x] = s;
}

// step s of BUILD: the largest gain, ties to the smallest x; record (x, -1, gain); D = min(D, q[x][.]).  One workgroup.
__global__ __launch_bounds__(BLOCK) void k_med_build_pick(const int32_t *__restrict__ q, int32_t n, int32_t ld, int32_t s, const long long *__restrict__ gain,
                                                          int32_t *__restrict__ D, int32_t *__restrict__ med, int32_t *__restrict__ is_med, long long *__restrict__ rec)
{
	__shared__ unsigned long long sh[2 * BLOCK / WAVE];
	long long best = INT64_MAX;
	uint32_t bx = UINT32_MAX, pay = 0;
	for (int32_t x = (int32_t)threadIdx.x; x < n; x += BLOCK) {
		const long long g = gain[x];
		if (g >= 0 && join_less(-g, (uint32_t)x, best, bx)) best = -g, bx = (uint32_t)x;
	}
	join_block_min(best, bx, pay, sh);
	const int32_t x = (int32_t)bx; // (k <= n - 1: there is always a candidate)
	if (threadIdx.x == 0) med[s] = x, is_med[x] = s, rec[3 * s] = x, rec[3 * s + 1] = -1, rec[3 * s + 2] = -best;
	const int32_t *row = q + (size_t)x * (size_t)ld;
	for (int32_t o = (int32_t)threadIdx.x; o < n; o += BLOCK) D[o] = min(D[o], row[o]);
}

// D, DS, NN of every column from the k medoid rows; removal[NN] += DS - D, cnt[NN] += 1 (both zero on entry).  stat == NULL: always runs
__global__ __launch_bounds__(BLOCK) void k_med_assign(const int32_t *__restrict__ q, int32_t n, int32_t ld, int32_t k, const int32_t *__restrict__ med,
                                                      int32_t *__restrict__ D, int32_t *__restrict__ DS, uint16_t *__restrict__ NN, long long *__restrict__ removal,
                                                      int32_t *__restrict__ cnt, const MedStat *__restrict__ stat)
{
	if (stat != nullptr && stat->done) return;
	const int32_t o = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	if (o >= n) return;
	int32_t d1 = MED_LIMIT, d2 = MED_LIMIT, nn = 0;
	for (int32_t s = 0; s < k; ++s) {
		const int32_t d = q[(size_t)med[s] * (size_t)ld + o];
		if (d < d1) d2 = d1, d1 = d, nn = s;
		else if (d < d2) d2 = d;
	}
	D[o] = d1, DS[o] = d2, NN[o] = (uint16_t)nn;
	if (d2 != d1) atomicAdd((unsigned long long *)&removal[nn], (unsigned long long)(d2 - d1));
	atomicAdd(&cnt[nn], 1);
}

// perm = the columns sorted by NN (counting sort; the order inside a cluster is whatever the atomics give, and nothing depends on it).
// Every workgroup scans cnt for itself -- where each cluster starts lives in its LDS alone, the row walk finds the boundaries from
// NN[perm[i]]; fill[] is zero on entry.  stat == NULL: always runs
__global__ __launch_bounds__(BLOCK) void k_med_scatter(int32_t n, int32_t k, const uint16_t *__restrict__ NN, const int32_t *__restrict__ cnt, int32_t *__restrict__ fill,
                                                       int32_t *__restrict__ perm, const MedStat *__restrict__ stat)
{
	__shared__ int32_t sh_seg[MED_MAX_K];
	__shared__ int32_t sh_wave[BLOCK / WAVE];
	if (stat != nullptr && stat->done) return;
	constexpr int PER = MED_MAX_K / BLOCK;
	const int t = (int)threadIdx.x;
	int32_t c[PER], tot = 0;
#pragma unroll
	for (int e = 0; e < PER; ++e) c[e] = t * PER + e < k ? cnt[t * PER + e] : 0, tot += c[e];
	int32_t inc = tot; // inclusive scan of the threads' totals over the wave
#pragma unroll
	for (int o = 1; o < WAVE; o <<= 1) {
		const int32_t v = __shfl_up(inc, o, WAVE);
		if (t % WAVE >= o) inc += v;
	}
	if (t % WAVE == WAVE - 1) sh_wave[t / WAVE] = inc;
	__syncthreads();
	int32_t base = inc - tot;
	for (int w = 0; w < t / WAVE; ++w) base += sh_wave[w];
#pragma unroll
	for (int e = 0; e < PER; ++e) sh_seg[t * PER + e] = base, base += c[e];
	__syncthreads();
	const int32_t o = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	if (o >= n) return;
	const int32_t cl = NN[o];
	perm[sh_seg[cl] + atomicAdd(&fill[cl], 1)] = o;
}

// The segmented row walk both the swap step and the sums use.  Workgroup (tile, chunk): lane = candidate x of the tile, rows
// perm[i0 .. i1) of the chunk.  SWAP: acc[NN][x] and plus[x] of the decomposition above; otherwise acc[NN][x] += q[row][x].
template <bool SWAP>
__device__ __forceinline__ void med_walk_body(const int32_t *__restrict__ q, int32_t n, int32_t ld, int32_t rows, const int32_t *__restrict__ perm,
                                              const uint16_t *__restrict__ NN, const int32_t *__restrict__ D, const int32_t *__restrict__ DS, long long *__restrict__ acc,
                                              long long *__restrict__ plus)
{
	const int32_t x = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	const int32_t i0 = (int32_t)blockIdx.y * rows, i1 = min(i0 + rows, n);
	if (i0 >= i1) return;
	const bool on = x < n;
	const int32_t xc = on ? x : 0; // a lane past the end reads column 0 and adds nothing
	long long a = 0, p = 0;
	int32_t cur = NN[perm[i0]];
	for (int32_t i = i0; i < i1; i += MED_BATCH) {
		int32_t cl[MED_BATCH], d[MED_BATCH], dn[MED_BATCH], ds[MED_BATCH];
#pragma unroll
		for (int e = 0; e < MED_BATCH; ++e) { // (the row and what is read per row are the same in every lane)
			const int32_t o = perm[min(i + e, i1 - 1)];
			cl[e] = NN[o];
			if (SWAP) dn[e] = D[o], ds[e] = DS[o];
			d[e] = q[(size_t)o * (size_t)ld + xc];
		}
#pragma unroll
		for (int e = 0; e < MED_BATCH; ++e) {
			if (i + e >= i1) break;
			if (cl[e] != cur) {
				if (on && a != 0) atomicAdd((unsigned long long *)&acc[(size_t)cur * (size_t)n + x], (unsigned long long)a);
				a = 0, cur = cl[e];
			}
			if (SWAP) {
				if (d[e] < dn[e]) p += d[e] - dn[e], a += dn[e] - ds[e];
				else if (d[e] < ds[e]) a += d[e] - ds[e];
			} else a += d[e];
		}
	}
	if (on && a != 0) atomicAdd((unsigned long long *)&acc[(size_t)cur * (size_t)n + x], (unsigned long long)a);
	if (SWAP && on && p != 0) atomicAdd((unsigned long long *)&plus[x], (unsigned long long)p);
}

__global__ __launch_bounds__(BLOCK) void k_med_swap(const int32_t *__restrict__ q, int32_t n, int32_t ld, int32_t rows, const int32_t *__restrict__ perm,
                                                    const uint16_t *__restrict__ NN, const int32_t *__restrict__ D, const int32_t *__restrict__ DS, long long *__restrict__ acc,
                                                    long long *__restrict__ plus, const MedStat *__restrict__ stat)
{
	if (stat->done) return;
	med_walk_body<true>(q, n, ld, rows, perm, NN, D, DS, acc, plus);
}

__global__ __launch_bounds__(BLOCK) void k_med_sums(const int32_t *__restrict__ q, int32_t n, int32_t ld, int32_t rows, const int32_t *__restrict__ perm,
                                                    const uint16_t *__restrict__ NN, long long *__restrict__ acc)
{
	med_walk_body<false>(q, n, ld, rows, perm, NN, nullptr, nullptr, acc, nullptr);
}

// per candidate x: the smallest (delta, medoid as assembly index) over the slots; acc and plus are cleared on the way
__global__ __launch_bounds__(BLOCK) void k_med_best(int32_t n, int32_t k, const int32_t *__restrict__ med, const int32_t *__restrict__ is_med,
                                                    const long long *__restrict__ removal, long long *__restrict__ acc, long long *__restrict__ plus,
                                                    long long *__restrict__ cand, int32_t *__restrict__ cand_slot, const MedStat *__restrict__ stat)
{
	if (stat->done) return;
	const int32_t x = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	if (x >= n) return;
	const long long p = plus[x];
	plus[x] = 0;
	long long best = INT64_MAX;
	int32_t bm = INT32_MAX, bs = 0;
	for (int32_t s = 0; s < k; ++s) {
		const size_t at = (size_t)s * (size_t)n + x;
		const long long a = acc[at];
		if (a != 0) acc[at] = 0;
		const long long dl = removal[s] + a + p;
		const int32_t m = med[s];
		if (dl < best || (dl == best && m < bm)) best = dl, bm = m, bs = s;
	}
	cand[x] = is_med[x] >= 0 ? INT64_MAX : best;
	cand_slot[x] = bs;
}

// the smallest (delta, x): not negative -> done; otherwise the swap, its record, and removal / cnt / fill cleared for k_med_assign.
// rec: the records of this chunk of iterations, base = the swaps before the chunk.  One workgroup.
__global__ __launch_bounds__(BLOCK) void k_med_pick(int32_t n, int32_t k, const long long *__restrict__ cand, const int32_t *__restrict__ cand_slot,
                                                    int32_t *__restrict__ med, int32_t *__restrict__ is_med, long long *__restrict__ removal, int32_t *__restrict__ cnt,
                                                    int32_t *__restrict__ fill, long long *__restrict__ rec, int32_t base, MedStat *__restrict__ stat)
{
	__shared__ unsigned long long sh[2 * BLOCK / WAVE];
	const int32_t was_done = stat->done;
	long long best = INT64_MAX;
	uint32_t bx = UINT32_MAX, pay = 0;
	if (!was_done)
		for (int32_t x = (int32_t)threadIdx.x; x < n; x += BLOCK) {
			const long long c = cand[x];
			if (join_less(c, (uint32_t)x, best, bx)) best = c, bx = (uint32_t)x, pay = (uint32_t)cand_slot[x];
		}
	join_block_min(best, bx, pay, sh); // (its barriers also order the read of `done` above before the write below)
	if (was_done) return;
	if (best >= 0) { if (threadIdx.x == 0) stat->done = 1; return; }
	if (threadIdx.x == 0) {
		const int32_t x = (int32_t)bx, s = (int32_t)pay, m = med[s];
		long long *r = rec + 3 * (size_t)(stat->n_swap - base);
		r[0] = x, r[1] = m, r[2] = best;
		med[s] = x, is_med[m] = -1, is_med[x] = s;
		stat->n_swap += 1;
	}
	for (int32_t s = (int32_t)threadIdx.x; s < k; s += BLOCK) removal[s] = 0, cnt[s] = 0, fill[s] = 0;
}

// The finish.  Clusters are the medoids in ascending order: smed[c], is_med[medoid] = c; cnt / fill / td cleared.  One workgroup.
__global__ __launch_bounds__(BLOCK) void k_med_rank(int32_t k, const int32_t *__restrict__ med, int32_t *__restrict__ smed, int32_t *__restrict__ is_med,
                                                    int32_t *__restrict__ cnt, int32_t *__restrict__ fill, long long *__restrict__ td)
{
	for (int32_t s = (int32_t)threadIdx.x; s < k; s += BLOCK) {
		const int32_t m = med[s];
		int32_t r = 0;
		for (int32_t t = 0; t < k; ++t) r += med[t] < m;
		smed[r] = m, is_med[m] = r, cnt[s] = 0, fill[s] = 0;
	}
	if (threadIdx.x == 0) *td = 0;
}

// label: a medoid its own cluster, any other column the medoid with the smallest (q, assembly index); dist, the cluster counts, td
__global__ __launch_bounds__(BLOCK) void k_med_label(const int32_t *__restrict__ q, int32_t n, int32_t ld, int32_t k, const int32_t *__restrict__ smed,
                                                     const int32_t *__restrict__ is_med, int32_t *__restrict__ label, int32_t *__restrict__ dist, uint16_t *__restrict__ NN,
                                                     int32_t *__restrict__ cnt, long long *__restrict__ td)
{
	const int32_t o = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	long long mine = 0;
	if (o < n) {
		int32_t c = is_med[o], d = 0;
		if (c < 0) {
			d = MED_LIMIT;
			for (int32_t s = 0; s < k; ++s) {
				const int32_t v = q[(size_t)smed[s] * (size_t)ld + o];
				if (v < d) d = v, c = s;
			}
		}
		label[o] = c, dist[o] = d, NN[o] = (uint16_t)c;
		atomicAdd(&cnt[c], 1);
		mine = d;
	}
#pragma unroll
	for (int x = WAVE / 2; x > 0; x >>= 1) mine += __shfl_xor(mine, x, WAVE);
	if (threadIdx.x % WAVE == 0 && mine != 0) atomicAdd((unsigned long long *)td, (unsigned long long)mine);
}

// sums[o][c] = acc[c][o], size[c] = cnt[c]
__global__ __launch_bounds__(BLOCK) void k_med_out(int32_t n, int32_t k, const long long *__restrict__ acc, const int32_t *__restrict__ cnt, long long *__restrict__ sums,
                                                   int32_t *__restrict__ size)
{
	const int32_t o = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	if (blockIdx.x == 0)
		for (int32_t c = (int32_t)threadIdx.x; c < k; c += BLOCK) size[c] = cnt[c];
	if (o >= n) return;
	for (int32_t c = 0; c < k; ++c) sums[(size_t)o * (size_t)k + c] = acc[(size_t)c * (size_t)n + o];
}
