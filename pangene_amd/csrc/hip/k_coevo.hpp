// ------------------------------------------------------------------------------------------------
// Co-evolution (pga_pan_coevo, include/pangene_hip.h; DESIGN.md section 8 "Co-evolution"): the item pairs whose gains and losses fall on the
// same branches.  The reconstruction is k_gainloss.hpp's (k_gl_up, k_gl_down, unchanged); every op but the last has one branch above its
// node, so a branch is named by its op k < B = n_op - 1.
//   k_ce_flag   events[g] = gains + losses of item g (gene[g][1], [2]) and its eligibility flag; a device scan of the flags gives every
//               eligible item its place among the E eligible ones (place[g], -1 for the others) and the map back.
//   k_ce_rows   the chunk's node-major state rows -- one 64-item ballot word per node -- into item-major event rows over the branches:
//               rows[place][plane][WB], plane 0 the gains, plane 1 the losses, WB = ceil(B / 32) words.  One workgroup per 64-item word
//               and span of CE_SPAN = 1 024 branches.  Lane l of a wave holds the gain and loss words of branch k (st[k] & ~st[par[k]] and
//               the reverse: bit i = item i), and 64 ballots per plane turn the 64 x 64 bits over: ballot i is item i's word over the 64
//               branches, kept by lane i.  The words go to LDS ([item][plane][32 words], rows 66 words apart so that the 8-byte writes of
//               64 lanes fall on distinct bank pairs), and from there 32 consecutive lanes write the 128 contiguous bytes a row's plane
//               has in this span.  Only eligible items have a row; a 64-item word without one ends at once.  Bits past B are zero because
//               the lanes of ops >= B hold zeros, and a row has no words past WB.
//   k_ce_pairs  one workgroup per 128 x 128 tile of the upper triangle of E x E, staging and micro-tile as BIT_TILE (k_dist.hpp: 32-word K
//               chunks in LDS rows of 36 words, 16 x 16 threads of 8 x 8 pairs each), over two planes: four staged blocks (G and L of the
//               row block, G and L of the column block: 73 728 B, two workgroups per CU) and two accumulators per pair,
//               same += popc(Gi & Gj) + popc(Li & Lj), opp += popc(Gi & Lj) + popc(Li & Gj).  The inner step reads two words per row
//               and plane (ds_read_b64), not four: 128 accumulators and 4 x 8 x 2 operand registers stay below the 256 VGPRs that two
//               workgroups per CU leave a thread.  The epilogue is k_assoc_pairs' scheme with a plain 64-bit test,
//               10^6 d^2 >= p^2 e_i e_j (d = same - opp; both sides below 2^54): per-workgroup count, one atomicAdd per workgroup,
//               records while the slot is below the capacity (key = place of i << eb | place of j, so[slot] = (same, opp), val = slot),
//               the counter counts everything.  The keys are radix-sorted and k_ce_emit writes (i, j, same, opp) with item numbers.
// The rows are dense: an item's events are few among B branches, and a sparse enumeration per branch is deliberately left out.
// ------------------------------------------------------------------------------------------------
constexpr int32_t CE_SPAN = 1024;                 // branches of one workgroup of k_ce_rows: 32 words per plane
constexpr int32_t CE_SPAN_W = CE_SPAN / 32;
constexpr int32_t CE_LDW = 2 * CE_SPAN_W + 2;     // LDS words of one item's two planes, padded
constexpr int32_t CE_LDS_WORDS = 4 * DIST_SIDE;   // k_ce_pairs: four staged blocks

__global__ __launch_bounds__(BLOCK) void k_ce_flag(const int32_t *__restrict__ gene, int32_t G, int32_t min_events, int32_t *__restrict__ events, int32_t *__restrict__ flag)
{
	const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (g >= G) return;
	const int32_t e = gene[(size_t)g * 4 + 1] + gene[(size_t)g * 4 + 2];
	events[g] = e, flag[g] = e >= min_events ? 1 : 0;
}

// output functor of the scan over the flags: eligible item i takes place excl; the last element leaves the total
struct OutCoevoMap {
	const int32_t *flag; int32_t *map, *place, *n_elig; int64_t n;
	__device__ __forceinline__ void operator()(int64_t i, I32 in, I32 ex) const
	{
		place[i] = flag[i] ? ex.v : -1;
		if (flag[i]) map[ex.v] = (int32_t)i;
		if (i == n - 1) *n_elig = in.v;
	}
};

// ce[e] = events[map[e]]
__global__ __launch_bounds__(BLOCK) void k_ce_gather(const int32_t *__restrict__ events, const int32_t *__restrict__ map, int32_t E, int32_t *__restrict__ ce)
{
	const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (e < E) ce[e] = events[map[e]];
}

// grid: (WC, ceil(B / CE_SPAN)).  st[n_op][WC] of the chunk that starts at item g0 and has Gc items; par[n_op]; place[G]; rows[E][2][WB]
__global__ __launch_bounds__(BLOCK) void k_ce_rows(const unsigned long long *__restrict__ st, const int32_t *__restrict__ par, const int32_t *__restrict__ place,
                                                   int32_t g0, int32_t Gc, int32_t B, int32_t WC, int32_t WB, uint32_t *__restrict__ rows)
{
	__shared__ uint2 sh2[64 * CE_LDW / 2];
	__shared__ int32_t pl[64];
	uint32_t *sh = (uint32_t *)sh2;
	const int32_t t = (int32_t)threadIdx.x, lane = t & (WAVE - 1), wave = t >> 6;
	const int32_t w = (int32_t)blockIdx.x, k_lo = (int32_t)blockIdx.y * CE_SPAN;
	int32_t mine = -1;
	if (t < 64) {
		const int32_t c = w * 64 + t;
		mine = c < Gc ? place[g0 + c] : -1;
		pl[t] = mine;
	}
	if (__syncthreads_or(mine >= 0) == 0) return; // no eligible item in this word
	// each wave: 4 of the span's 16 groups of 64 branches
#pragma unroll 1
	for (int32_t q = 0; q < CE_SPAN / 64 / (BLOCK / WAVE); ++q) {
		const int32_t grp = wave + (BLOCK / WAVE) * q, k = k_lo + grp * 64 + lane;
		unsigned long long gw = 0, lw = 0;
		if (k < B) {
			const unsigned long long s = st[(size_t)k * (size_t)WC + (size_t)w], p = st[(size_t)par[k] * (size_t)WC + (size_t)w];
			gw = s & ~p, lw = ~s & p;
		}
		unsigned long long ig = 0, il = 0; // item `lane`'s words over the group's 64 branches
#pragma unroll 8
		for (int32_t i = 0; i < 64; ++i) {
			const unsigned long long bg = __ballot((gw >> i) & 1ull), bl = __ballot((lw >> i) & 1ull);
			if (lane == i) ig = bg, il = bl;
		}
		*(uint2 *)(sh + lane * CE_LDW + grp * 2) = make_uint2((uint32_t)ig, (uint32_t)(ig >> 32));
		*(uint2 *)(sh + lane * CE_LDW + CE_SPAN_W + grp * 2) = make_uint2((uint32_t)il, (uint32_t)(il >> 32));
	}
	__syncthreads();
	const int32_t w_lo = k_lo / 32;
#pragma unroll 1
	for (int32_t e = t; e < 64 * 2 * CE_SPAN_W; e += BLOCK) {
		const int32_t r = e >> 6, plane = (e >> 5) & 1, c = e & 31, at = pl[r];
		if (at >= 0 && w_lo + c < WB) rows[((size_t)at * 2 + (size_t)plane) * (size_t)WB + (size_t)(w_lo + c)] = sh[r * CE_LDW + plane * CE_SPAN_W + c];
	}
}

struct CoevoPar {
	int32_t E, WB, n_chunk, sign, eb; // eb: bits of a place (key = place of i << eb | place of j)
	uint32_t p2;                      // p^2
	int64_t cap;                      // records the buffers hold
};

// grid: the T (T + 1) / 2 upper-triangle tiles of E x E.  rows[E][2][WB], ce[E]
__global__ __launch_bounds__(BLOCK, 2) void k_ce_pairs(const uint32_t *__restrict__ rows, const int32_t *__restrict__ ce, const CoevoPar par,
                                                      unsigned long long *__restrict__ counter, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals,
                                                      uint2 *__restrict__ so)
{
	__shared__ uint4 sh4[CE_LDS_WORDS / 4];
	__shared__ I32 wave_tot[BLOCK / WAVE];
	__shared__ unsigned long long base_s;
	uint32_t *sh = (uint32_t *)sh4;
	const int32_t t = (int32_t)threadIdx.x, tx = t & 15, ty = t >> 4;
	const int32_t E = par.E, WB = par.WB;
	int32_t ti, tj;
	dist_tile_of((int32_t)blockIdx.x, ti, tj);
	const int32_t i0 = ti * DIST_TILE, j0 = tj * DIST_TILE;

	uint32_t same[8][8], opp[8][8];
#pragma unroll
	for (int32_t ii = 0; ii < 8; ++ii)
#pragma unroll
		for (int32_t jj = 0; jj < 8; ++jj) same[ii][jj] = 0, opp[ii][jj] = 0;
	// blocks 0, 1: G and L of the row block; 2, 3: G and L of the column block
	const uint32_t *sag = sh, *sal = sh + DIST_SIDE, *sbg = sh + 2 * DIST_SIDE, *sbl = sh + 3 * DIST_SIDE;
	for (int32_t c = 0; c < par.n_chunk; ++c) {
		// word e = t + BLOCK * r of a block's chunk at row e >> 5, word e & 31, so 32 lanes read one 128-byte row piece
#pragma unroll 1
		for (int32_t blk = 0; blk < 4; ++blk) { // (not unrolled: one block's 16 loads in flight, and no 64 addresses kept across the chunks)
			uint32_t v[DIST_LOADS / 2];
			const int32_t g0 = blk >= 2 ? j0 : i0, plane = blk & 1;
			// a uniform base and a 32-bit offset per thread: row r of the thread is 8 rows = 16 WB words further on
			const uint32_t *src = rows + ((size_t)g0 * 2 + (size_t)plane) * (size_t)WB + (size_t)(c * DIST_KC);
			const uint32_t off = (uint32_t)(t >> 5) * 2u * (uint32_t)WB + (uint32_t)(t & 31);
			const bool k_in = c * DIST_KC + (t & 31) < WB;
#pragma unroll
			for (int32_t r = 0; r < DIST_LOADS / 2; ++r)
				v[r] = (k_in && g0 + (t >> 5) + 8 * r < E) ? src[off + (uint32_t)r * 16u * (uint32_t)WB] : 0u;
			if (blk == 0 && c > 0) __syncthreads(); // everyone is done with the previous chunk
#pragma unroll
			for (int32_t r = 0; r < DIST_LOADS / 2; ++r) {
				const int32_t e = t + BLOCK * r;
				sh[blk * DIST_SIDE + (e >> 5) * DIST_LDW + (e & 31)] = v[r];
			}
		}
		__syncthreads();
		const int32_t kk_hi = min(DIST_KC, (WB - c * DIST_KC + 1) & ~1);
#pragma unroll 1
		for (int32_t kk = 0; kk < kk_hi; kk += 2) {
			uint2 ag[8], al[8], bg[8], bl[8];
#pragma unroll
			for (int32_t ii = 0; ii < 8; ++ii) {
				ag[ii] = *(const uint2 *)(sag + (ty + 16 * ii) * DIST_LDW + kk);
				al[ii] = *(const uint2 *)(sal + (ty + 16 * ii) * DIST_LDW + kk);
			}
#pragma unroll
			for (int32_t jj = 0; jj < 8; ++jj) {
				bg[jj] = *(const uint2 *)(sbg + (tx + 16 * jj) * DIST_LDW + kk);
				bl[jj] = *(const uint2 *)(sbl + (tx + 16 * jj) * DIST_LDW + kk);
			}
#pragma unroll
			for (int32_t ii = 0; ii < 8; ++ii)
#pragma unroll
				for (int32_t jj = 0; jj < 8; ++jj) {
					uint32_t x = same[ii][jj], y = opp[ii][jj];
					x = __popc(ag[ii].x & bg[jj].x) + x; asm volatile("" : "+v"(x));
					x = __popc(al[ii].x & bl[jj].x) + x; asm volatile("" : "+v"(x));
					x = __popc(ag[ii].y & bg[jj].y) + x; asm volatile("" : "+v"(x));
					x = __popc(al[ii].y & bl[jj].y) + x; asm volatile("" : "+v"(x));
					y = __popc(ag[ii].x & bl[jj].x) + y; asm volatile("" : "+v"(y));
					y = __popc(al[ii].x & bg[jj].x) + y; asm volatile("" : "+v"(y));
					y = __popc(ag[ii].y & bl[jj].y) + y; asm volatile("" : "+v"(y));
					y = __popc(al[ii].y & bg[jj].y) + y; asm volatile("" : "+v"(y));
					same[ii][jj] = x, opp[ii][jj] = y;
				}
		}
	}

	// the epilogue: e of the thread's 8 rows and 8 columns, then the 64 tests
	uint32_t ej[8];
#pragma unroll
	for (int32_t jj = 0; jj < 8; ++jj) {
		const int32_t gj = j0 + tx + 16 * jj;
		ej[jj] = gj < E ? (uint32_t)ce[gj] : 0u;
	}
	uint64_t valid = 0; // the pairs of this thread that exist: both rows eligible items, and i < j on a diagonal tile
#pragma unroll
	for (int32_t ii = 0; ii < 8; ++ii)
#pragma unroll
		for (int32_t jj = 0; jj < 8; ++jj) {
			const int32_t li = ty + 16 * ii, lj = tx + 16 * jj;
			valid |= (uint64_t)(i0 + li < E && j0 + lj < E && (ti != tj || li < lj)) << (ii * 8 + jj);
		}
	asm volatile("" : "+v"(valid)); // (as one mask in two registers, not as 64 lane masks in scalar registers)
	uint64_t sel = 0;
#pragma unroll
	for (int32_t ii = 0; ii < 8; ++ii) {
		const int32_t li = ty + 16 * ii;
		const uint64_t ei = i0 + li < E ? (uint64_t)ce[i0 + li] : 0u;
#pragma unroll
		for (int32_t jj = 0; jj < 8; ++jj) {
			uint32_t s = same[ii][jj], o = opp[ii][jj];
			asm volatile("" : "+v"(s), "+v"(o)); // one pair after the other: 64 pairs' 64-bit products at once do not fit the registers
			const int64_t d = (int64_t)s - (int64_t)o;
			const bool ok = par.sign == 0 || (par.sign == 1) == (d >= 0);
			const bool pass = (uint64_t)(d * d) * 1000000ull >= ei * (uint64_t)ej[jj] * (uint64_t)par.p2;
			sel |= (uint64_t)(ok && pass) << (ii * 8 + jj);
			asm volatile("" : "+v"(sel));
		}
	}
	sel &= valid;

	I32 tot;
	const I32 ex = block_scan_excl(I32{(int32_t)__popcll(sel)}, OpSum{}, I32{0}, wave_tot, &tot);
	if (tot.v == 0) return;
	if (t == 0) base_s = atomicAdd(counter, (unsigned long long)tot.v);
	__syncthreads();
	int64_t slot = (int64_t)base_s + ex.v;
#pragma unroll
	for (int32_t ii = 0; ii < 8; ++ii)
#pragma unroll
		for (int32_t jj = 0; jj < 8; ++jj)
			if (sel >> (ii * 8 + jj) & 1) {
				if (slot < par.cap) {
					keys[slot] = (uint64_t)(i0 + ty + 16 * ii) << par.eb | (uint64_t)(j0 + tx + 16 * jj);
					vals[slot] = (uint32_t)slot;
					so[slot] = make_uint2(same[ii][jj], opp[ii][jj]);
				}
				++slot;
			}
}

// the sorted records with the original item numbers: out[i] = (map[place of i], map[place of j], same, opp)
__global__ __launch_bounds__(BLOCK) void k_ce_emit(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const uint2 *__restrict__ so, int64_t n, int32_t eb,
                                                   const int32_t *__restrict__ map, int32_t *__restrict__ out)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n) return;
	const uint64_t k = keys[i];
	const uint2 v = so[vals[i]];
	out[i * 4] = map[k >> eb], out[i * 4 + 1] = map[k & ((1ull << eb) - 1)], out[i * 4 + 2] = (int32_t)v.x, out[i * 4 + 3] = (int32_t)v.y;
}
