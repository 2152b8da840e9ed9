// ------------------------------------------------------------------------------------------------
// Phylogenetic signal (pga_pan_phylosig, include/pangene_hip.h; DESIGN.md section 8 "Phylogenetic signal"): the permutation tail of the
// parsimony cost.  The null distribution of an item depends only on its number of carriers, so the replicates are classes x permutations:
// replicate (n, p) has assembly x present iff o_p[x] < n, o_p the pinned order of k_perm.hpp.
//   k_ps_ranks  the orders of one batch, assembly-major: rk[x][nbs], the value of permutation q of the batch at rk[x * nbs + q].  One
//               lane per permutation over a private row that starts as 0 .. n_leaf - 1 (perm_wave_block: the wave's rows already stand
//               in this layout, so the write-out is a copy).
//   k_ps_cost   the hot kernel: k_gl_up's walk of the postfix program, a lane being one permutation that carries CLS classes in
//               registers.  The top entry lives in registers, the ones below in LDS, lane-interleaved: value c of class j of entry e of
//               lane l at ((e * CLS + j) * 2 + c) * PS_BLOCK + l.  A push loads r = rk[leaf[k] * nbs + q], one 128-byte line per wave,
//               and class j has the tip present iff r < cls[c0 + j].  No ballots, no decision rows: only the root's min(C0, C1) is
//               kept, as cost[(c0 + j) * B + q], and the wave's sum goes into sum[c0 + j] with one unsigned 64-bit atomicAdd per class
//               (the adds commute: the sum does not depend on scheduling).
//   k_ps_count  one wave per item: the lanes stride over the row of the item's class, compare with the observed cost and popcount the
//               two ballots; lane 0 adds into n_le[i] and n_ge[i].  A wave owns its item and the batches follow each other on one
//               stream, so the add is a plain load, add and store.
// Lanes past nb and class slots past n_cls run a valid replicate (the last column of rk, the last class) and write nothing.
// ------------------------------------------------------------------------------------------------
constexpr int32_t PS_BLOCK = 128;           // lanes (permutations) of a workgroup of k_ps_cost: two waves
constexpr int32_t PS_RANK_LDS_N = 256;      // leaves up to which a wave's 64 orders stay in LDS (32 KiB)
constexpr int32_t PS_COUNT_BLOCK = 256;     // k_ps_count: four waves, four items

// grid: ceil(nb / 64) workgroups of ONE wave.  rk[n_leaf][nbs], nbs = 64 * gridDim.x; work[workgroup][n_leaf][64] when !USE_LDS
template <bool USE_LDS>
__global__ __launch_bounds__(WAVE) void k_ps_ranks(int32_t n_leaf, uint32_t seed, uint32_t p0, int32_t nbs, uint16_t *__restrict__ work, uint16_t *__restrict__ rk)
{
	perm_wave_block<uint16_t, PS_RANK_LDS_N, USE_LDS>(
		n_leaf, n_leaf, seed, p0, work, [](int32_t k) { return (uint16_t)k; }, PermSwapValues(), rk, (size_t)nbs);
}

// grid: (ceil(nb / 128), ceil(n_cls / CLS)).  ops[ceil(n_op / 32)], leaf[n_leaf], rk[n_leaf][nbs], cls[n_cls], cost[n_cls][B], sum[n_cls];
// dynamic LDS: max(depth - 1, 1) * 2 * PS_BLOCK * CLS words
template <int32_t CLS>
__global__ __launch_bounds__(PS_BLOCK) void k_ps_cost(const uint32_t *__restrict__ ops, const int32_t *__restrict__ leaf_of, const uint16_t *__restrict__ rk,
                                                      const int32_t *__restrict__ cls, int32_t n_cls, int32_t n_op, int32_t gain, int32_t loss, int32_t nb,
                                                      int32_t nbs, int32_t B, int32_t *__restrict__ cost, unsigned long long *__restrict__ sum)
{
	extern __shared__ int32_t ps_stack[];
	const int32_t l = (int32_t)threadIdx.x;
	const int32_t q = (int32_t)blockIdx.x * PS_BLOCK + l;
	const bool mine = q < nb;
	const uint16_t *my_rk = rk + (size_t)min(q, nbs - 1);
	const int32_t c0 = (int32_t)blockIdx.y * CLS;
	int32_t n[CLS], t0[CLS], t1[CLS]; // the classes' sizes; the top entry
#pragma unroll
	for (int32_t j = 0; j < CLS; ++j) n[j] = cls[min(c0 + j, n_cls - 1)], t0[j] = 0, t1[j] = 0;
	int32_t sp = 0, leaf = 0; // entries on the stack, leaves pushed: both wave-uniform
	uint32_t op_word = 0;
	for (int32_t k = 0; k < n_op; ++k) {
		if ((k & 31) == 0) op_word = ops[k >> 5];
		if (((op_word >> (k & 31)) & 1u) == 0) { // push
			const int32_t r = (int32_t)my_rk[(size_t)leaf_of[leaf] * (size_t)nbs];
			if (sp > 0) {
				int32_t *e = ps_stack + (sp - 1) * CLS * 2 * PS_BLOCK + l;
#pragma unroll
				for (int32_t j = 0; j < CLS; ++j) e[(j * 2) * PS_BLOCK] = t0[j], e[(j * 2 + 1) * PS_BLOCK] = t1[j];
			}
#pragma unroll
			for (int32_t j = 0; j < CLS; ++j) {
				const bool b = r < n[j];
				t0[j] = b ? gain + loss : 0, t1[j] = b ? 0 : gain + loss;
			}
			++sp, ++leaf;
		} else { // join the entry below the top with the top
			const int32_t *e = ps_stack + (sp - 2) * CLS * 2 * PS_BLOCK + l;
#pragma unroll
			for (int32_t j = 0; j < CLS; ++j) {
				const int32_t l0 = e[(j * 2) * PS_BLOCK], l1 = e[(j * 2 + 1) * PS_BLOCK];
				const int32_t n0 = min(l0, l1 + gain) + min(t0[j], t1[j] + gain), n1 = min(l1, l0 + loss) + min(t1[j], t0[j] + loss);
				t0[j] = n0, t1[j] = n1;
			}
			--sp;
		}
	}
#pragma unroll
	for (int32_t j = 0; j < CLS; ++j) {
		const int32_t c = min(t0[j], t1[j]);
		const bool row = c0 + j < n_cls; // (block-uniform)
		if (row && mine) cost[(size_t)(c0 + j) * (size_t)B + (size_t)q] = c;
		const unsigned long long s = wave_sum64(mine ? (unsigned long long)c : 0ull);
		if (row && (l & (WAVE - 1)) == 0 && s != 0) atomicAdd(sum + (c0 + j), s);
	}
}

// grid: ceil(n_item / 4).  cost[n_cls][B] of a batch of nb permutations; n_le[i], n_ge[i] += the batch's counts
__global__ __launch_bounds__(PS_COUNT_BLOCK) void k_ps_count(const int32_t *__restrict__ cost, const int32_t *__restrict__ item_cls, const int32_t *__restrict__ item_cost,
                                                             int32_t n_item, int32_t nb, int32_t B, int32_t *__restrict__ n_le, int32_t *__restrict__ n_ge)
{
	const int32_t lane = (int32_t)threadIdx.x & (WAVE - 1);
	const int32_t i = (int32_t)blockIdx.x * (PS_COUNT_BLOCK / WAVE) + ((int32_t)threadIdx.x >> 6);
	if (i >= n_item) return; // (the whole wave)
	const int32_t *row = cost + (size_t)item_cls[i] * (size_t)B;
	const int32_t obs = item_cost[i];
	int32_t le = 0, ge = 0; // wave-uniform
	for (int32_t q0 = 0; q0 < nb; q0 += WAVE) {
		const int32_t q = q0 + lane;
		const int32_t c = row[min(q, nb - 1)];
		le += __popcll(__ballot(q < nb && c <= obs)), ge += __popcll(__ballot(q < nb && c >= obs));
	}
	if (lane == 0) n_le[i] += le, n_ge[i] += ge;
}
