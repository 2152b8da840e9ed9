// ------------------------------------------------------------------------------------------------
// Lineage-aware pairwise comparisons (pga_pan_pairs, include/pangene_hip.h; DESIGN.md section 8 "Lineage-aware trait test"): one tree
// dynamic programme per (gene, label row, run).  Every gene runs the SAME postfix program over the tree -- push the next leaf, join the
// top two entries -- so a wave's control flow is uniform and a lane differs only in its data: one lane per gene, blockIdx.y = label row,
// blockIdx.z = run (0: ties go to the supporting pairs, 1: to the opposing ones).
//   value   pairs << 15 | pairs of the run's side.  n_leaf <= 65 535, so pairs <= 32 767: a feasible value, and the sum of two siblings'
//           values, stays below 2^30 and the side never carries into the pairs.  Infeasible is any negative value, stored as
//           >= PAIRS_NONE = -2^30: the sum of two stored values is then >= -2^31 (no wrap), and a feasible plus an infeasible one is
//           still negative.
//   entry   N and F[4] (type = gene bit * 2 + label: 3 and 0 support, 2 and 1 oppose).  The top entry lives in registers, the ones
//           below in LDS, lane-interleaved: value c of entry e of lane l at (e * 5 + c) * PAIRS_BLOCK + l, so a wave reads and writes
//           one conflict-free row of 64 dwords.  The LDS is sized per launch by the depth the program needs (the host knows it):
//           (depth - 1) * 5 * 128 * 4 bytes, 37.5 KiB at the depth limit of 16, 12.5 KiB for the 6 a balanced tree of 32 leaves needs.
//   inputs  the program is a bit string (32 ops a word) and the label row two bit planes (has a value, is 1; 32 leaves a word): the host
//           packs them, every lane of a wave reads the same word, so they come through the scalar cache once per 32 ops / leaves.  The
//           gene bits stay as pan_shared lays them out: every 32 leaves a lane gathers its bit of the next 32 rows (two distinct words a
//           wave and row, 32 independent loads in flight) into one register.
// ------------------------------------------------------------------------------------------------
constexpr int32_t PAIRS_BLOCK = 128;         // lanes (genes) of a workgroup: two waves
constexpr int32_t PAIRS_DEPTH = 16;          // stack entries a program may need
constexpr int32_t PAIRS_NONE = -(1 << 30);   // infeasible, as stored
constexpr int32_t PAIRS_SHIFT = 15;
constexpr int32_t PAIRS_MAX_LEAF = 65535, PAIRS_MAX_GENE = 16777215;

// grid: (ceil(G / 128), rows of this launch, 2).  ops[ceil(n_op / 32)], bits[n_leaf][W], has / one[n_row][LW] with LW = ceil(n_leaf / 32),
// out[n_row][G][3]; dynamic LDS: max(depth - 1, 1) * 5 * PAIRS_BLOCK words
__global__ __launch_bounds__(PAIRS_BLOCK) void k_pairs(const uint32_t *__restrict__ ops, const uint32_t *__restrict__ bits, const uint32_t *__restrict__ has,
                                                       const uint32_t *__restrict__ one, int32_t G, int32_t W, int32_t n_leaf, int32_t LW, int32_t n_op,
                                                       int32_t row0, int32_t *__restrict__ out)
{
	extern __shared__ int32_t pairs_stack[];
	const int32_t l = (int32_t)threadIdx.x;
	const int32_t g = (int32_t)blockIdx.x * PAIRS_BLOCK + l;
	const int32_t gc = min(g, G - 1); // lanes past G run gene G - 1 again and write nothing
	const int32_t row = row0 + (int32_t)blockIdx.y, run = (int32_t)blockIdx.z;
	const uint32_t *my_bits = bits + (size_t)(gc >> 5);
	const uint32_t *row_has = has + (size_t)row * (size_t)LW, *row_one = one + (size_t)row * (size_t)LW;
	const int32_t add_supp = (1 << PAIRS_SHIFT) + (run == 0 ? 1 : 0), add_opp = (1 << PAIRS_SHIFT) + (run == 0 ? 0 : 1);

	int32_t tN = 0, tF0 = PAIRS_NONE, tF1 = PAIRS_NONE, tF2 = PAIRS_NONE, tF3 = PAIRS_NONE; // the top entry
	int32_t sp = 0, leaf = 0;                                                              // entries on the stack, leaves pushed: both wave-uniform
	uint32_t op_word = 0, has_word = 0, one_word = 0, gene_word = 0;
	for (int32_t k = 0; k < n_op; ++k) {
		if ((k & 31) == 0) op_word = ops[k >> 5];
		if (((op_word >> (k & 31)) & 1u) == 0) { // push
			if ((leaf & 31) == 0) {
				has_word = row_has[leaf >> 5], one_word = row_one[leaf >> 5];
				gene_word = 0;
#pragma unroll
				for (int32_t j = 0; j < 32; ++j) {
					const int32_t r = min(leaf + j, n_leaf - 1);
					gene_word |= ((my_bits[(size_t)r * (size_t)W] >> (gc & 31)) & 1u) << j;
				}
			}
			if (sp > 0) {
				int32_t *e = pairs_stack + (sp - 1) * 5 * PAIRS_BLOCK + l;
				e[0] = tN, e[PAIRS_BLOCK] = tF0, e[2 * PAIRS_BLOCK] = tF1, e[3 * PAIRS_BLOCK] = tF2, e[4 * PAIRS_BLOCK] = tF3;
			}
			const uint32_t b = leaf & 31;
			const bool typed = (has_word >> b) & 1u;
			const int32_t type = (int32_t)(((gene_word >> b) & 1u) * 2u + ((one_word >> b) & 1u));
			tN = 0;
			tF0 = typed && type == 0 ? 0 : PAIRS_NONE, tF1 = typed && type == 1 ? 0 : PAIRS_NONE;
			tF2 = typed && type == 2 ? 0 : PAIRS_NONE, tF3 = typed && type == 3 ? 0 : PAIRS_NONE;
			++sp, ++leaf;
		} else { // join the entry below the top with the top
			const int32_t *e = pairs_stack + (sp - 2) * 5 * PAIRS_BLOCK + l;
			const int32_t lN = e[0], lF0 = e[PAIRS_BLOCK], lF1 = e[2 * PAIRS_BLOCK], lF2 = e[3 * PAIRS_BLOCK], lF3 = e[4 * PAIRS_BLOCK];
			int32_t n = lN + tN;
			n = max(n, max(lF3 + tF0, lF0 + tF3) + add_supp);
			n = max(n, max(lF2 + tF1, lF1 + tF2) + add_opp);
			tF0 = max(max(lF0 + tN, lN + tF0), PAIRS_NONE), tF1 = max(max(lF1 + tN, lN + tF1), PAIRS_NONE);
			tF2 = max(max(lF2 + tN, lN + tF2), PAIRS_NONE), tF3 = max(max(lF3 + tN, lN + tF3), PAIRS_NONE);
			tN = n;
			--sp;
		}
	}
	if (g < G) {
		int32_t *o = out + ((size_t)row * (size_t)G + (size_t)g) * 3;
		if (run == 0) o[0] = tN >> PAIRS_SHIFT, o[1] = tN & ((1 << PAIRS_SHIFT) - 1);
		else o[2] = tN & ((1 << PAIRS_SHIFT) - 1);
	}
}
