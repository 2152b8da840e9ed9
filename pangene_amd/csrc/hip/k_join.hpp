// k_join.hpp -- the joins of pangene tree (pga_pan_join, include/pangene_hip.h): neighbour-joining and UPGMA over a fixed-point distance
// matrix.  Included by pga_backend.hip; uses BLOCK / WAVE from there.
//
// Storage.  The live matrix is kept compact: the r live slots sit at positions 0 .. r - 1 of an int32 matrix d[.][ld] (ld = n rounded
// up to 4, so that every row starts on 16 bytes), and after a join the last live position moves into the one that retired.  label[p] is
// the slot number of the definition that position p holds; every tie compares labels, never positions.  aux[p] is R (NJ: the sum of
// the row over the live positions) or the leaf count (UPGMA), int64.
//
// A join is two launches.  k_join_argmin<NJ> covers the upper triangle (by position) in tiles of JOIN_RB rows x JOIN_CW columns, a
// fixed number of workgroups striding over the tiles: a lane keeps four columns' aux and labels in registers and walks down the rows
// with 16-byte loads, so a wave reads 1 KiB of a row at a time and the per-row values are wave-uniform.  The criterion is int64,
// (criterion, label i << 16 | label j) is compared lexicographically (labels stay below 2^16), and one candidate per workgroup goes
// to part[] with the pair's distance and aux values beside it.  k_join_update<NJ> has one thread per live position: every workgroup
// reduces part[] for itself, the thread of position k rewrites (keep, k) and (k, keep), moves (last, k) into the retired position,
// and carries R along with integer adds (the new node's R by 64-bit atomics, which commute).  Nothing it reads is written by another
// thread of the launch: the winning pair's positions, distance and aux values come from part[], rows pi / pj / last are read at column k by
// thread k alone, and the writes go to (keep, .), (drop, .) and columns keep / drop of rows no thread reads.
#pragma once

constexpr int JOIN_RB = 16;          // rows of a tile
constexpr int JOIN_CW = BLOCK * 4;   // columns of a tile: four per lane
constexpr int JOIN_MAX_PART = 1024;  // candidates a step leaves: workgroups of k_join_argmin
constexpr int32_t JOIN_IN_LIMIT = 1 << 29, JOIN_LIMIT = 1 << 30;

struct JoinPart { // one workgroup's candidate; crit = INT64_MAX: none
	long long crit;
	uint32_t key;  // label i << 16 | label j, label i < label j
	uint32_t pos;  // position of label i << 16 | position of label j
	long long aux_i, aux_j; // aux of the positions holding label i / label j
	int32_t d, pad;
};

__device__ __forceinline__ bool join_less(long long c, uint32_t k, long long bc, uint32_t bk) { return c < bc || (c == bc && k < bk); }
__device__ __forceinline__ long long join_floor_div(long long a, long long b) { const long long q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; }

// (crit, key, payload) -> the smallest of the workgroup in every thread; sh: 2 * BLOCK / WAVE words of 64 bits
__device__ __forceinline__ void join_block_min(long long &c, uint32_t &k, uint32_t &p, unsigned long long *sh)
{
#pragma unroll
	for (int o = WAVE / 2; o > 0; o >>= 1) {
		const long long oc = __shfl_xor(c, o, WAVE);
		const uint32_t ok = __shfl_xor(k, o, WAVE), op = __shfl_xor(p, o, WAVE);
		if (join_less(oc, ok, c, k)) c = oc, k = ok, p = op;
	}
	const int w = threadIdx.x / WAVE;
	__syncthreads(); // (sh may still be read from an earlier call)
	if (threadIdx.x % WAVE == 0) sh[w] = (unsigned long long)c, sh[BLOCK / WAVE + w] = (unsigned long long)k << 32 | p;
	__syncthreads();
	c = (long long)sh[0], k = (uint32_t)(sh[BLOCK / WAVE] >> 32), p = (uint32_t)sh[BLOCK / WAVE];
#pragma unroll
	for (int x = 1; x < BLOCK / WAVE; ++x) {
		const long long oc = (long long)sh[x];
		const uint32_t ok = (uint32_t)(sh[BLOCK / WAVE + x] >> 32), op = (uint32_t)sh[BLOCK / WAVE + x];
		if (join_less(oc, ok, c, k)) c = oc, k = ok, p = op;
	}
}

// The kernels' bodies are device functions, so that the single-tree kernels and their batched twins (one replicate per blockIdx.y, every
// array at a stride; pga_pan_boot, k_boot.hpp) are the same code.

// label[p] = p, aux[p] = R or 1, flag |= an entry out of the input range.  One workgroup per row.
template <bool NJ>
__device__ __forceinline__ void join_init_body(const int32_t *__restrict__ d, int32_t n, int32_t ld, int32_t *__restrict__ label, long long *__restrict__ aux,
                                               int32_t *__restrict__ flag)
{
	__shared__ unsigned long long sh[BLOCK / WAVE];
	const int32_t row = (int32_t)blockIdx.x;
	const int32_t *p = d + (size_t)row * (size_t)ld;
	long long s = 0;
	bool bad = false;
	for (int32_t c = (int32_t)threadIdx.x; c < n; c += BLOCK) {
		const int32_t v = p[c];
		s += v;
		bad |= v >= JOIN_IN_LIMIT || v <= -JOIN_IN_LIMIT;
	}
	if (bad) *flag = 1;
	if (NJ) {
#pragma unroll
		for (int o = WAVE / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, WAVE);
		if (threadIdx.x % WAVE == 0) sh[threadIdx.x / WAVE] = (unsigned long long)s;
		__syncthreads();
		if (threadIdx.x == 0) {
			unsigned long long t = 0;
			for (int x = 0; x < BLOCK / WAVE; ++x) t += sh[x];
			aux[row] = (long long)t;
		}
	} else if (threadIdx.x == 0) aux[row] = 1;
	if (threadIdx.x == 0) label[row] = row;
}

template <bool NJ>
__global__ __launch_bounds__(BLOCK) void k_join_init(const int32_t *__restrict__ d, int32_t n, int32_t ld, int32_t *__restrict__ label, long long *__restrict__ aux,
                                                     int32_t *__restrict__ flag)
{
	join_init_body<NJ>(d, n, ld, label, aux, flag);
}

template <bool NJ>
__device__ __forceinline__ void join_argmin_body(const int32_t *__restrict__ d, int32_t ld, int32_t r, const int32_t *__restrict__ label,
                                                 const long long *__restrict__ aux, JoinPart *__restrict__ part)
{
	__shared__ unsigned long long sh[2 * BLOCK / WAVE];
	const int32_t n_cc = (r + JOIN_CW - 1) / JOIN_CW, n_rb = (r + JOIN_RB - 1) / JOIN_RB, n_tile = n_cc * n_rb;
	const long long m = (long long)r - 2;
	long long best = INT64_MAX;
	uint32_t bkey = UINT32_MAX, bpos = 0;
	for (int32_t t = (int32_t)blockIdx.x; t < n_tile; t += (int32_t)gridDim.x) {
		const int32_t rb = t / n_cc, cc = t - rb * n_cc;
		const int32_t a0 = rb * JOIN_RB, c_lo = cc * JOIN_CW;
		if (c_lo + JOIN_CW - 1 <= a0) continue; // the whole tile is on or below the diagonal
		const int32_t c = c_lo + (int32_t)threadIdx.x * 4; // this lane's columns c .. c + 3 (inside the row's ld words whenever c < r)
		const int32_t a1 = min(a0 + JOIN_RB, r);
		const bool lane_on = c < r;
		long long xb[4];
		uint32_t lb[4];
#pragma unroll
		for (int e = 0; e < 4; ++e) {
			const bool in = c + e < r;
			xb[e] = NJ && in ? aux[c + e] : 0;
			lb[e] = in ? (uint32_t)label[c + e] : 0u;
		}
#pragma unroll 4
		for (int32_t a = a0; a < a1; ++a) { // (a and what is read per row are the same in every lane)
			const int4 v4 = lane_on ? *(const int4 *)(d + (size_t)a * (size_t)ld + c) : make_int4(0, 0, 0, 0);
			const int32_t v[4] = {v4.x, v4.y, v4.z, v4.w};
			const long long xa = NJ ? aux[a] : 0;
			const uint32_t la = (uint32_t)label[a];
#pragma unroll
			for (int e = 0; e < 4; ++e) {
				const int32_t b = c + e;
				if (b <= a || b >= r) continue;
				const long long crit = NJ ? m * (long long)v[e] - xa - xb[e] : (long long)v[e];
				if (crit > best) continue;
				const uint32_t key = la < lb[e] ? la << 16 | lb[e] : lb[e] << 16 | la;
				if (join_less(crit, key, best, bkey)) best = crit, bkey = key, bpos = (uint32_t)a << 16 | (uint32_t)b;
			}
		}
	}
	join_block_min(best, bkey, bpos, sh);
	if (threadIdx.x == 0) {
		JoinPart o;
		o.crit = best, o.key = bkey, o.pos = bpos, o.aux_i = o.aux_j = 0, o.d = 0, o.pad = 0;
		if (best != INT64_MAX) {
			const int32_t a = (int32_t)(bpos >> 16), b = (int32_t)(bpos & 0xffffu);
			const bool a_is_i = (uint32_t)label[a] == bkey >> 16;
			o.pos = a_is_i ? bpos : (uint32_t)b << 16 | (uint32_t)a;
			o.d = d[(size_t)a * (size_t)ld + b];
			o.aux_i = aux[a_is_i ? a : b], o.aux_j = aux[a_is_i ? b : a];
		}
		part[blockIdx.x] = o;
	}
}

template <bool NJ>
__global__ __launch_bounds__(BLOCK) void k_join_argmin(const int32_t *__restrict__ d, int32_t ld, int32_t r, const int32_t *__restrict__ label,
                                                       const long long *__restrict__ aux, JoinPart *__restrict__ part)
{
	join_argmin_body<NJ>(d, ld, r, label, aux, part);
}

// step s of the run: record s, the new row and column, R, the compaction, the range flag.  One thread per live position.
template <bool NJ>
__device__ __forceinline__ void join_update_body(int32_t *__restrict__ d, int32_t ld, int32_t r, int32_t *__restrict__ label, long long *__restrict__ aux,
                                                 const JoinPart *__restrict__ part, int32_t n_part, long long *__restrict__ rec, int32_t *__restrict__ flag)
{
	__shared__ unsigned long long sh[2 * BLOCK / WAVE];
	long long best = INT64_MAX;
	uint32_t bkey = UINT32_MAX, bidx = 0;
	for (int32_t x = (int32_t)threadIdx.x; x < n_part; x += BLOCK) {
		const long long c = part[x].crit;
		const uint32_t k = part[x].key;
		if (join_less(c, k, best, bkey)) best = c, bkey = k, bidx = (uint32_t)x;
	}
	join_block_min(best, bkey, bidx, sh);
	const JoinPart w = part[bidx];
	const int32_t pi = (int32_t)(w.pos >> 16), pj = (int32_t)(w.pos & 0xffffu), last = r - 1;
	const int32_t li = (int32_t)(w.key >> 16), lj = (int32_t)(w.key & 0xffffu);
	// the new node stays at pi and the last live position moves into pj -- unless pi is the last one itself: then the node goes to pj
	const int32_t keep = pi == last ? pj : pi, drop = pi == last ? pi : pj;
	const long long dij = w.d, xi = w.aux_i, xj = w.aux_j;
	const int32_t k = (int32_t)(blockIdx.x * BLOCK + threadIdx.x);
	if (k == 0) { rec[0] = li, rec[1] = lj, rec[2] = dij, rec[3] = xi, rec[4] = xj, rec[5] = r; }
	long long add = 0; // what this thread adds to the new node's R
	if (k < r && k != pi && k != pj) {
		const long long da = d[(size_t)pi * (size_t)ld + k], db = d[(size_t)pj * (size_t)ld + k];
		const long long v = NJ ? (da + db - dij) >> 1 : join_floor_div(xi * da + xj * db, xi + xj);
		if (v >= JOIN_LIMIT || v <= -JOIN_LIMIT) *flag = 1;
		const int32_t to = k == last ? drop : k; // where position k is after the step (k == last only when drop != last: pi, pj are excluded)
		d[(size_t)keep * (size_t)ld + to] = (int32_t)v;
		d[(size_t)to * (size_t)ld + keep] = (int32_t)v;
		if (NJ) {
			aux[to] = aux[k] + v - da - db;
			add = v;
		} else if (k == last) aux[to] = aux[k];
		if (k == last) label[to] = label[k];
		else if (drop != last) {
			const int32_t dl = d[(size_t)last * (size_t)ld + k];
			d[(size_t)drop * (size_t)ld + k] = dl;
			d[(size_t)k * (size_t)ld + drop] = dl;
		}
	} else if (k == keep) {
		label[keep] = li;
		if (NJ) add = -(keep == pi ? xi : xj); // R of the new node = the sum of the new row: the old R leaves, the adds arrive in any order
		else aux[keep] = xi + xj;
	}
	if (NJ) {
#pragma unroll
		for (int o = WAVE / 2; o > 0; o >>= 1) add += __shfl_xor(add, o, WAVE);
		if (threadIdx.x % WAVE == 0 && add != 0) atomicAdd((unsigned long long *)&aux[keep], (unsigned long long)add);
	}
}

template <bool NJ>
__global__ __launch_bounds__(BLOCK) void k_join_update(int32_t *__restrict__ d, int32_t ld, int32_t r, int32_t *__restrict__ label, long long *__restrict__ aux,
                                                       const JoinPart *__restrict__ part, int32_t n_part, long long *__restrict__ rec, int32_t *__restrict__ flag)
{
	join_update_body<NJ>(d, ld, r, label, aux, part, n_part, rec, flag);
}

// NJ's closing record at r = 3: the live slots x < y < z and their three distances
__device__ __forceinline__ void join_final_body(const int32_t *__restrict__ d, int32_t ld, const int32_t *__restrict__ label, long long *__restrict__ rec)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	int32_t p[3] = {0, 1, 2};
	for (int x = 0; x < 2; ++x)
		for (int y = 0; y + 1 < 3 - x; ++y)
			if (label[p[y]] > label[p[y + 1]]) { const int32_t t = p[y]; p[y] = p[y + 1]; p[y + 1] = t; }
	rec[0] = label[p[0]], rec[1] = label[p[1]], rec[2] = label[p[2]];
	rec[3] = d[(size_t)p[0] * (size_t)ld + p[1]], rec[4] = d[(size_t)p[0] * (size_t)ld + p[2]], rec[5] = d[(size_t)p[1] * (size_t)ld + p[2]];
}

__global__ void k_join_final(const int32_t *__restrict__ d, int32_t ld, const int32_t *__restrict__ label, long long *__restrict__ rec)
{
	join_final_body(d, ld, label, rec);
}

// The batched twins: replicate blockIdx.y of a bootstrap chunk.  All replicates have the same n, ld and live count r, so one launch
// serves a step of every replicate; d is d_stride words apart, label and aux v_stride entries, part p_stride candidates, rec
// rec_stride words, and the flags are one word each.
template <bool NJ>
__global__ __launch_bounds__(BLOCK) void k_join_init_b(const int32_t *__restrict__ d, int32_t n, int32_t ld, int32_t *__restrict__ label, long long *__restrict__ aux,
                                                       int32_t *__restrict__ flag, size_t d_stride, int32_t v_stride)
{
	const size_t q = blockIdx.y;
	join_init_body<NJ>(d + q * d_stride, n, ld, label + q * (size_t)v_stride, aux + q * (size_t)v_stride, flag + q);
}

template <bool NJ>
__global__ __launch_bounds__(BLOCK) void k_join_argmin_b(const int32_t *__restrict__ d, int32_t ld, int32_t r, const int32_t *__restrict__ label,
                                                         const long long *__restrict__ aux, JoinPart *__restrict__ part, size_t d_stride, int32_t v_stride,
                                                         int32_t p_stride)
{
	const size_t q = blockIdx.y;
	join_argmin_body<NJ>(d + q * d_stride, ld, r, label + q * (size_t)v_stride, aux + q * (size_t)v_stride, part + q * (size_t)p_stride);
}

template <bool NJ>
__global__ __launch_bounds__(BLOCK) void k_join_update_b(int32_t *__restrict__ d, int32_t ld, int32_t r, int32_t *__restrict__ label, long long *__restrict__ aux,
                                                         const JoinPart *__restrict__ part, int32_t n_part, long long *__restrict__ rec, int32_t *__restrict__ flag,
                                                         size_t d_stride, int32_t v_stride, int32_t p_stride, size_t rec_stride)
{
	const size_t q = blockIdx.y;
	join_update_body<NJ>(d + q * d_stride, ld, r, label + q * (size_t)v_stride, aux + q * (size_t)v_stride, part + q * (size_t)p_stride, n_part,
	                     rec + q * rec_stride, flag + q);
}

__global__ void k_join_final_b(const int32_t *__restrict__ d, int32_t ld, const int32_t *__restrict__ label, long long *__restrict__ rec, size_t d_stride,
                               int32_t v_stride, size_t rec_stride)
{
	const size_t q = blockIdx.y;
	join_final_body(d + q * d_stride, ld, label + q * (size_t)v_stride, rec + q * rec_stride);
}
