// ------------------------------------------------------------------------------------------------
// Gene associations (pga_pan_assoc): the transpose of k_dist.hpp -- an all-pairs popcount over GENE bit rows -- that selects on the
// device.  Three steps:
//   prepare  k_assoc_count: |B_g| of every row (8 lanes a row) and the eligibility flag; a device scan of the flags gives every
//            eligible row its place among the E eligible ones (the map back to the original row is written by the scan's output
//            functor); k_assoc_gather copies the eligible rows next to each other.  In a U-shaped pangenome most genes are core or
//            rare, so E << G and the E^2 work below is a small part of G^2.
//   pairs    k_assoc_pairs: one workgroup per 128 x 128 tile of the upper triangle of E x E, the tile body of k_dist_shared (BIT_TILE: 32-word
//            K chunks of the two row blocks in LDS, 8 x 8 micro-tile per thread, v_and_b32 + v_bcnt_u32_b32 with the empty asm that
//            keeps the compiler from regrouping the adds).  Two differences: the inner loop stops at the last word of the rows (at
//            200 assemblies that is 8 words of the 32-word chunk), and there is no split K -- the epilogue needs finished counts, and
//            when the tiles are too few to fill the device the whole job is small.
//   epilogue every thread tests its 64 finished counts s against 10^6 D^2 >= p^2 V_g V_h (D = s A - a b).  The decision is exact:
//            a double-precision test with a guard band settles the pairs that are clearly inside or outside, and only a pair inside
//            the band takes the 128-bit integer comparison.  D is exact in double (s A and a b are below 2^48 and the fma rounds an
//            exactly representable result), L = D * D, R = V_g * (V_h * (p^2 / 10^6)): four roundings in all, so L / R is off its
//            true value by less than 2^-50 relative, and the band is 2^-40 on either side.  There is no a * b + c in the test that a
//            contraction could fuse differently (the only fused operation is the explicit, exact fma).  The survivors are counted per
//            workgroup (popcount of the thread's 64-bit mask, block scan), ONE global atomicAdd per workgroup reserves the slots, and
//            the records (key = place of g << eb | place of h, value = s) go out with ordinary stores while the slot is below the
//            capacity; the counter counts everything, so when it ends above the capacity the host grows the buffers and runs the
//            kernel once more.  The keys are then radix-sorted (dev_prims.hpp), so the order of the atomics never shows, and
//            k_assoc_emit writes (g, h, s) with the original row numbers.
// ------------------------------------------------------------------------------------------------
constexpr int32_t ASSOC_ROW_LANES = 8; // lanes that share one row in k_assoc_count
constexpr double ASSOC_BAND = 1.0 / 1099511627776.0; // 2^-40

__global__ __launch_bounds__(BLOCK) void k_assoc_count(const uint32_t *__restrict__ bits, int32_t G, int32_t W, int32_t A, int32_t min_count,
                                                       int32_t *__restrict__ count, int32_t *__restrict__ flag)
{
	const int64_t g = (int64_t)blockIdx.x * (BLOCK / ASSOC_ROW_LANES) + (int64_t)(threadIdx.x / ASSOC_ROW_LANES);
	const int32_t l = (int32_t)threadIdx.x % ASSOC_ROW_LANES;
	int32_t a = 0;
	if (g < G) {
		const uint32_t *row = bits + (size_t)g * (size_t)W;
		for (int32_t k = l; k < W; k += ASSOC_ROW_LANES) a += __popc(row[k]);
	}
	a = row8_sum(a);
	if (g < G && l == 0) count[g] = a, flag[g] = min(a, A - a) >= min_count ? 1 : 0;
}

// output functor of the scan over the flags: eligible row i takes place excl; the last element leaves the total
struct OutAssocMap {
	const int32_t *flag; int32_t *map, *n_elig; int64_t n;
	__device__ __forceinline__ void operator()(int64_t i, I32 in, I32 ex) const
	{
		if (flag[i]) map[ex.v] = (int32_t)i;
		if (i == n - 1) *n_elig = in.v;
	}
};

// cbits[e][W] = bits[map[e]][W], ca[e] = count[map[e]]; grid-stride over the E * W words
__global__ __launch_bounds__(BLOCK) void k_assoc_gather(const uint32_t *__restrict__ bits, const int32_t *__restrict__ map, const int32_t *__restrict__ count,
                                                        int32_t E, int32_t W, uint32_t *__restrict__ cbits, int32_t *__restrict__ ca)
{
	const int64_t n = (int64_t)E * (int64_t)W, step = (int64_t)gridDim.x * BLOCK;
	for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += step) {
		const int64_t e = i / W, k = i - e * W;
		const int32_t g = map[e];
		cbits[i] = bits[(size_t)g * (size_t)W + (size_t)k];
		if (k == 0) ca[e] = count[g];
	}
}

// the definition, for the pairs inside the guard band: 10^6 D^2 >= p^2 V_g V_h with both sides below 2^112
__device__ __forceinline__ bool assoc_exact(int64_t D, int64_t Vg, int64_t Vh, uint32_t p2)
{
	typedef unsigned __int128 u128;
	const u128 d = (u128)(uint64_t)(D < 0 ? -D : D);
	return d * d * (u128)1000000u >= (u128)(uint64_t)Vg * (u128)(uint64_t)Vh * (u128)p2;
}

struct AssocPar {
	int32_t E, W, n_chunk, A, sign, eb; // eb: bits of a place (key = place of g << eb | place of h)
	uint32_t p2;                        // p^2
	double p2s;                         // p^2 / 10^6
	int64_t cap;                        // records the buffers hold
};

// grid: the T (T + 1) / 2 upper-triangle tiles of E x E
__global__ __launch_bounds__(BLOCK, 2) void k_assoc_pairs(const uint32_t *__restrict__ cbits, const int32_t *__restrict__ ca, const AssocPar par,
                                                         unsigned long long *__restrict__ counter, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
	__shared__ uint4 sh4[DIST_LDS_WORDS / 4];
	__shared__ I32 wave_tot[BLOCK / WAVE];
	__shared__ unsigned long long base_s;
	uint32_t *sh = (uint32_t *)sh4;
	const int32_t t = (int32_t)threadIdx.x, tx = t & 15, ty = t >> 4;
	const int32_t E = par.E, W = par.W;
	int32_t ti, tj;
	dist_tile_of((int32_t)blockIdx.x, ti, tj);
	const int32_t i0 = ti * DIST_TILE, j0 = tj * DIST_TILE;

	BIT_TILE(true, cbits, E, cbits, E, W, 0, par.n_chunk)

	// the epilogue: a and V of the thread's 8 rows and 8 columns, then the 64 tests
	const double Ad = (double)par.A;
	double bd[8], w[8];
#pragma unroll
	for (int32_t jj = 0; jj < 8; ++jj) {
		const int32_t gj = j0 + tx + 16 * jj;
		bd[jj] = gj < E ? (double)ca[gj] : 0.0;
		w[jj] = (bd[jj] * (Ad - bd[jj])) * par.p2s; // V_h exact (below 2^48), one rounding in the product
	}
	uint64_t valid = 0; // the pairs of this thread that exist: both rows eligible rows, and g < h on a diagonal tile
#pragma unroll
	for (int32_t ii = 0; ii < 8; ++ii)
#pragma unroll
		for (int32_t jj = 0; jj < 8; ++jj) {
			const int32_t li = ty + 16 * ii, lj = tx + 16 * jj;
			valid |= (uint64_t)(i0 + li < E && j0 + lj < E && (ti != tj || li < lj)) << (ii * 8 + jj);
		}
	asm volatile("" : "+v"(valid)); // (as one mask in two registers, not as 64 lane masks in scalar registers)
	uint64_t sel = 0, band = 0; // selected for certain; inside the guard band
#pragma unroll
	for (int32_t ii = 0; ii < 8; ++ii) {
		const int32_t li = ty + 16 * ii;
		const double ad = i0 + li < E ? (double)ca[i0 + li] : 0.0, u = ad * (Ad - ad); // V_g, exact
#pragma unroll
		for (int32_t jj = 0; jj < 8; ++jj) {
			uint32_t s = acc[ii][jj];
			asm volatile("" : "+v"(s)); // one pair after the other: 64 pairs' doubles at once do not fit the registers
			const double D = fma((double)s, Ad, -(ad * bd[jj])); // exact
			const double L = D * D, R = u * w[jj];
			const bool hi = L > R * (1.0 + ASSOC_BAND), lo = L < R * (1.0 - ASSOC_BAND);
			const bool ok = par.sign == 0 || (par.sign == 1) == (D >= 0.0);
			sel |= (uint64_t)(ok && hi) << (ii * 8 + jj);
			band |= (uint64_t)(ok && !hi && !lo) << (ii * 8 + jj);
		}
	}
	sel &= valid, band &= valid;
	// the pairs inside the band, one at a time (rare: the count comes out of the registers through a chain of selects)
	while (band) {
		const int32_t bit = __ffsll((unsigned long long)band) - 1;
		band &= band - 1;
		uint32_t s = 0;
#pragma unroll
		for (int32_t ii = 0; ii < 8; ++ii)
#pragma unroll
			for (int32_t jj = 0; jj < 8; ++jj) s = bit == ii * 8 + jj ? acc[ii][jj] : s;
		const int64_t a = ca[i0 + ty + 16 * (bit >> 3)], b = ca[j0 + tx + 16 * (bit & 7)], An = par.A;
		if (assoc_exact((int64_t)s * An - a * b, a * (An - a), b * (An - b), par.p2)) sel |= 1ull << bit;
	}

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
					vals[slot] = acc[ii][jj];
				}
				++slot;
			}
}

// the sorted records with the original row numbers: out[i] = (map[place of g], map[place of h], s)
__global__ __launch_bounds__(BLOCK) void k_assoc_emit(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, int64_t n, int32_t eb,
                                                      const int32_t *__restrict__ map, int32_t *__restrict__ out)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n) return;
	const uint64_t k = keys[i];
	out[i * 3] = map[k >> eb], out[i * 3 + 1] = map[k & ((1ull << eb) - 1)], out[i * 3 + 2] = (int32_t)vals[i];
}
