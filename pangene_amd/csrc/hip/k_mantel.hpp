// ------------------------------------------------------------------------------------------------
// Mantel test (pga_pan_mantel; DESIGN.md section 8 "Mantel test"): do two distance matrices of the same N assemblies agree.  With a and
// b the two shifted matrices (symmetric, zero diagonal), an order o of the assemblies gives Z(o) = sum over ordered pairs i != j of
// a[i][j] b[o[i]][o[j]]; Z_obs is Z of the identity, and n_ge / n_le count the permutations p with Z_p >= Z_obs / Z_p <= Z_obs.  Unlike
// k_perma_quad, which permutes a 0/1 label row and so is a matrix product, this permutes the assemblies themselves: per permutation
// N (N - 1) / 2 gathered multiply-adds, no matrix cores.
//   order  k_mantel_order: the orders of one batch as uint16 rows ord[p][N] (N <= 16 384).  One lane per permutation runs the pinned
//          swap sequence (k_perm.hpp) over a private row that starts as 0 .. N - 1.  The wave's 64 rows are laid out as k_perm.hpp says,
//          in LDS while they fit (N <= 256) and in a global scratch buffer beyond; the finished rows are written row-major.
//          identity: no swaps -- the observed matrix as a batch of one.
//   z      k_mantel_z: a workgroup takes one permutation and MZ_ROWS rows i of a.  It holds o_p in LDS (2 N bytes) and, per row, stages
//          row o[i] of b into LDS with coalesced loads (4 N bytes), reads a[i][j], j > i, coalesced from global, gathers row[o[j]] from
//          LDS and accumulates a b in 64 bits; the last row has no j > i and is not staged.  The workgroup's sum is reduced (wave_sum64,
//          then four partial sums in LDS) and added TWICE -- the pair (j, i) gives the same product -- with ONE 64-bit atomicAdd into
//          Z[p].  The adds are unsigned, so they wrap and commute; the total is below 2^62 (the caller's promise
//          max_a max_b N (N - 1) < 2^62), so Z does not depend on scheduling.  The LDS is dynamic, 64 + 6 N bytes: 96 KiB at N = 16 384,
//          12 KiB at N = 2 000, where eight workgroups share a CU and one's staging hides behind another's gathers.
//   stat   k_mantel_stat: Z_p against Z_obs (out[MT_Z]: the observed matrix goes through z and stat first, so it stands in device
//          memory before any count reads it), permutations past the batch masked, one atomicAdd per wave into n_ge and into n_le.  It
//          clears Z[p] behind itself for the next batch.
// ------------------------------------------------------------------------------------------------
constexpr int32_t MZ_ROWS = 16;               // rows of a per workgroup of k_mantel_z: o_p is loaded once for 16 staged rows (3 % on top)
constexpr int32_t MZ_LDS_HEAD = 64;           // bytes in front of the staged row: the waves' partial sums
constexpr int32_t MANTEL_ORDER_LDS_N = 256;   // columns up to which a wave's 64 orders stay in LDS (32 KiB)
enum { MT_Z = 0, MT_GE = 1, MT_LE = 2, MT_N_OUT = 3 }; // out[]: Z of the observed matrix, n_ge, n_le

// perm_wave_rows (k_perm.hpp) over rows of N indices: permutation p0 + q of the batch is row q of ord[nb][N].  USE_LDS: the wave's rows
// in LDS (N <= MANTEL_ORDER_LDS_N); otherwise in work[workgroup][N][64].  identity: no swaps.
template <bool USE_LDS>
__global__ __launch_bounds__(WAVE) void k_mantel_order(int32_t N, uint32_t seed, uint32_t p0, int32_t nb, bool identity, uint16_t *__restrict__ work,
                                                       uint16_t *__restrict__ ord)
{
	perm_wave_rows<uint16_t, MANTEL_ORDER_LDS_N, USE_LDS>(
		N, identity ? 0 : N, seed, p0, nb, work, [](int32_t k) { return (uint16_t)k; }, PermSwapValues(),
		[&](const uint16_t *fin, int64_t q, int32_t l) { perm_row_major(fin, ord + (size_t)q * (size_t)N, N, l); });
}

// grid: (nb, ceil((N - 1) / MZ_ROWS)), dynamic LDS: mantel_z_lds(N) bytes.  a[N][N], b[N][N], ord[nb][N] with every entry below N;
// z[p] += twice the share of the workgroup's rows in Z of permutation p of the batch
__global__ __launch_bounds__(BLOCK) void k_mantel_z(const int32_t *__restrict__ a, const int32_t *__restrict__ b, const uint16_t *__restrict__ ord, int32_t N,
                                                    unsigned long long *__restrict__ z)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char mz_lds[];
	unsigned long long *part = (unsigned long long *)mz_lds;
	int32_t *row = (int32_t *)(mz_lds + MZ_LDS_HEAD);
	uint16_t *o = (uint16_t *)(mz_lds + MZ_LDS_HEAD + 4 * (size_t)((N + 3) & ~3));
	const int32_t t = (int32_t)threadIdx.x, p = (int32_t)blockIdx.x;
	const int32_t i0 = (int32_t)blockIdx.y * MZ_ROWS, i1 = min(i0 + MZ_ROWS, N - 1); // (row N - 1 has no j > i)
	const uint16_t *op = ord + (size_t)p * (size_t)N;
	for (int32_t k = t; k < N; k += BLOCK) o[k] = op[k];
	unsigned long long sum = 0;
	for (int32_t i = i0; i < i1; ++i) {
		__syncthreads(); // o is there; the row of the round before is no longer read
		const int32_t *br = b + (size_t)o[i] * (size_t)N;
		for (int32_t k = t; k < N; k += BLOCK) row[k] = br[k];
		__syncthreads();
		const int32_t *ar = a + (size_t)i * (size_t)N;
#pragma unroll 4
		for (int32_t j = i + 1 + t; j < N; j += BLOCK) sum += (unsigned long long)((long long)ar[j] * (long long)row[o[j]]);
	}
	sum = wave_sum64(sum);
	if ((t & (WAVE - 1)) == 0) part[t / WAVE] = sum;
	__syncthreads();
	if (t == 0) {
		unsigned long long all = 0;
#pragma unroll
		for (int32_t k = 0; k < BLOCK / WAVE; ++k) all += part[k];
		// unsigned: the adds wrap and commute, the total is below 2^62 (see the head of this file)
		if (all != 0) atomicAdd(z + p, 2 * all);
	}
}

// grid: ceil(nb / 256).  observed: the batch is the identity order alone and out[MT_Z] is written; otherwise out[MT_GE] += #{p < nb :
// Z_p >= out[MT_Z]} and out[MT_LE] += #{p < nb : Z_p <= out[MT_Z]}.  z[p] is read and cleared.  z_rows: NULL, or (tests) Z_p of the batch
__global__ __launch_bounds__(BLOCK) void k_mantel_stat(unsigned long long *__restrict__ z, int32_t nb, bool observed, long long *__restrict__ out,
                                                       long long *__restrict__ z_rows)
{
	const int64_t p = (int64_t)blockIdx.x * BLOCK + (int64_t)threadIdx.x;
	bool ge = false, le = false;
	if (p < nb) {
		const long long zp = (long long)z[p];
		z[p] = 0;
		if (z_rows != nullptr) z_rows[p] = zp;
		if (observed) out[MT_Z] = zp;
		else ge = zp >= out[MT_Z], le = zp <= out[MT_Z];
	}
	const unsigned long long n_ge = __ballot(ge), n_le = __ballot(le);
	if ((threadIdx.x & (WAVE - 1)) == 0) {
		if (n_ge != 0) atomicAdd((unsigned long long *)(out + MT_GE), (unsigned long long)__popcll(n_ge));
		if (n_le != 0) atomicAdd((unsigned long long *)(out + MT_LE), (unsigned long long)__popcll(n_le));
	}
}
