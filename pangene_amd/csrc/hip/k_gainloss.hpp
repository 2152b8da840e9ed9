// ------------------------------------------------------------------------------------------------
// Gene gain and loss on a tree (pga_pan_gainloss, include/pangene_hip.h; DESIGN.md section 8 "Gain and loss"): Wagner parsimony per item
// over the postfix program k_pairs runs -- push the next leaf, join the top two entries -- one lane per item, uniform control flow.
// Every op makes exactly one node, so a node is named by its op index k, and everything per node is a row k of 64-bit words, one bit per
// item: word w of a row holds items 64 w .. 64 w + 63 of the chunk, which is one wave's ballot.
//   k_gl_up    the program forwards.  An entry is (C0, C1), the cheapest cost of the subtree with its root absent / present; the top entry
//              lives in registers, the ones below in LDS, lane-interleaved: value c of entry e of lane l at (e * 2 + c) * GL_BLOCK + l.
//              When a node's entry is complete the wave stores two ballots: k0[k] = "a child here switches under an absent parent",
//              k1[k] = "... under a present parent".  Row k of the root holds its state in both (C1 < C0), so the way down treats the
//              root as the child of an absent parent that switches exactly when it is present.  gene[g][0] = cost, gene[g][3] = root.
//   k_gl_down  the program backwards.  The stack of the reversed walk has the forward walk's sizes (<= 16) and its entries are one bit,
//              the state of a parent whose children are still to come: one register.  st[k] = the wave's states, gene[g][1], [2] =
//              the lane's gains and losses.
//   k_gl_node  one wave per row k: present = sum popc(st[k]), and against the parent's row the gains and losses on the branch above k,
//              added into node[k][3].  A row belongs to one wave and the launches of a call follow each other on one stream, so the
//              add is a plain load, add and store.
// Lanes past the chunk run its last item again and are masked out of every ballot, so their bits are zero in all three row arrays.
// ------------------------------------------------------------------------------------------------
constexpr int32_t GL_BLOCK = 128;            // lanes (items) of a workgroup of k_gl_up / k_gl_down: two waves
constexpr int32_t GL_DEPTH = 16;             // stack entries a program may need
constexpr int32_t GL_MAX_LEAF = 65535, GL_MAX_GENE = 16777215;
constexpr int32_t GL_NODE_BLOCK = 256;       // k_gl_node: four waves, four rows
constexpr int32_t GL_AHEAD = 8;              // k_gl_down: ops whose decision words are loaded ahead

// grid: ceil(Gc / 128).  ops[ceil(n_op / 32)], bits[n_leaf][W] of ALL items (the chunk starts at item g0, a multiple of 64, and has Gc
// items), k0 / k1[n_op][WW] with WW = ceil(Gc / 64), gene[G][4]; dynamic LDS: max(depth - 1, 1) * 2 * GL_BLOCK words
__global__ __launch_bounds__(GL_BLOCK) void k_gl_up(const uint32_t *__restrict__ ops, const uint32_t *__restrict__ bits, int32_t g0, int32_t Gc, int32_t W,
                                                     int32_t n_leaf, int32_t n_op, int32_t gain, int32_t loss, int32_t early, int32_t WW,
                                                     unsigned long long *__restrict__ k0, unsigned long long *__restrict__ k1, int32_t *__restrict__ gene)
{
	extern __shared__ int32_t gl_stack[];
	const int32_t l = (int32_t)threadIdx.x;
	const int32_t c = (int32_t)blockIdx.x * GL_BLOCK + l; // the item inside the chunk
	const bool mine = c < Gc;
	const int32_t g = g0 + min(c, Gc - 1);
	const int32_t word = c >> 6;
	const bool writer = (l & (WAVE - 1)) == 0 && word < WW;
	const uint32_t *my_bits = bits + (size_t)(g >> 5);

	int32_t t0 = 0, t1 = 0;   // the top entry
	int32_t sp = 0, leaf = 0; // entries on the stack, leaves pushed: both wave-uniform
	uint32_t op_word = 0, gene_word = 0;
	for (int32_t k = 0; k < n_op; ++k) {
		if ((k & 31) == 0) op_word = ops[k >> 5];
		if (((op_word >> (k & 31)) & 1u) == 0) { // push
			if ((leaf & 31) == 0) {
				gene_word = 0;
#pragma unroll
				for (int32_t j = 0; j < 32; ++j) {
					const int32_t r = min(leaf + j, n_leaf - 1);
					gene_word |= ((my_bits[(size_t)r * (size_t)W] >> (g & 31)) & 1u) << j;
				}
			}
			if (sp > 0) {
				int32_t *e = gl_stack + (sp - 1) * 2 * GL_BLOCK + l;
				e[0] = t0, e[GL_BLOCK] = t1;
			}
			const bool b = (gene_word >> (leaf & 31)) & 1u;
			t0 = b ? gain + loss : 0, t1 = b ? 0 : gain + loss;
			++sp, ++leaf;
		} else { // join the entry below the top with the top
			const int32_t *e = gl_stack + (sp - 2) * 2 * GL_BLOCK + l;
			const int32_t l0 = e[0], l1 = e[GL_BLOCK];
			const int32_t n0 = min(l0, l1 + gain) + min(t0, t1 + gain), n1 = min(l1, l0 + loss) + min(t1, t0 + loss);
			t0 = n0, t1 = n1;
			--sp;
		}
		bool s0, s1; // the node switches under an absent / a present parent
		if (k == n_op - 1) s0 = s1 = t1 < t0;
		else if (early) s0 = t1 + gain <= t0, s1 = t0 + loss <= t1;
		else s0 = t1 + gain < t0, s1 = t0 + loss < t1;
		const unsigned long long b0 = __ballot(mine && s0), b1 = __ballot(mine && s1);
		if (writer) k0[(size_t)k * (size_t)WW + (size_t)word] = b0, k1[(size_t)k * (size_t)WW + (size_t)word] = b1;
	}
	if (mine) {
		const int32_t root = t1 < t0;
		gene[(size_t)g * 4] = root ? t1 : t0, gene[(size_t)g * 4 + 3] = root;
	}
}

// grid: ceil(Gc / 128).  st[n_op][WW]
__global__ __launch_bounds__(GL_BLOCK) void k_gl_down(const uint32_t *__restrict__ ops, int32_t g0, int32_t Gc, int32_t n_op, int32_t WW,
                                                       const unsigned long long *__restrict__ k0, const unsigned long long *__restrict__ k1,
                                                       unsigned long long *__restrict__ st, int32_t *__restrict__ gene)
{
	const int32_t l = (int32_t)threadIdx.x;
	const int32_t c = (int32_t)blockIdx.x * GL_BLOCK + l;
	const bool mine = c < Gc;
	const int32_t word = c >> 6, bit = c & 63;
	const bool in_rows = word < WW; // (a wave wholly past the chunk has no word)
	const bool writer = (l & (WAVE - 1)) == 0 && in_rows;

	uint32_t stack = 0; // bit 0 = the top: the state of the parent of the node visited next (under the root: absent)
	int32_t gains = 0, losses = 0;
	uint32_t op_word = 0;
	// A visit needs one word of k0 or k1, and which one hangs on the state before: read one at a time, every op would wait for a load.
	// The addresses do not hang on the states, so both words of the next GL_AHEAD ops are loaded before the first of them is visited.
	for (int32_t kb = n_op - 1; kb >= 0; kb -= GL_AHEAD) {
		unsigned long long w0[GL_AHEAD], w1[GL_AHEAD];
#pragma unroll
		for (int32_t j = 0; j < GL_AHEAD; ++j) {
			const size_t at = (size_t)max(kb - j, 0) * (size_t)WW + (size_t)word;
			w0[j] = in_rows ? k0[at] : 0ull, w1[j] = in_rows ? k1[at] : 0ull;
		}
#pragma unroll
		for (int32_t j = 0; j < GL_AHEAD; ++j) {
			const int32_t k = kb - j;
			if (k < 0) break;
			if (k == n_op - 1 || (k & 31) == 31) op_word = ops[k >> 5];
			const uint32_t p = stack & 1u;
			stack >>= 1;
			const uint32_t s = p ^ (uint32_t)(((p ? w1[j] : w0[j]) >> bit) & 1ull);
			if (k != n_op - 1) gains += (int32_t)(s & ~p), losses += (int32_t)(p & ~s);
			const unsigned long long b = __ballot(mine && s);
			if (writer) st[(size_t)k * (size_t)WW + (size_t)word] = b;
			if ((op_word >> (k & 31)) & 1u) stack = stack << 2 | s * 3u; // a join: both children see this state
		}
	}
	if (mine) {
		const int32_t g = g0 + c;
		gene[(size_t)g * 4 + 1] = gains, gene[(size_t)g * 4 + 2] = losses;
	}
}

// grid: ceil(n_op / 4).  par[n_op] = the op of the parent, -1 for the root; node[n_op][3] += present, gains, losses of the chunk
__global__ __launch_bounds__(GL_NODE_BLOCK) void k_gl_node(const unsigned long long *__restrict__ st, const int32_t *__restrict__ par, int32_t n_op, int32_t WW,
                                                            long long *__restrict__ node)
{
	const int32_t lane = (int32_t)threadIdx.x & (WAVE - 1);
	const int32_t k = (int32_t)blockIdx.x * (GL_NODE_BLOCK / WAVE) + ((int32_t)threadIdx.x >> 6);
	if (k >= n_op) return;
	const int32_t up = par[k];
	const unsigned long long *row = st + (size_t)k * (size_t)WW, *prow = st + (size_t)max(up, 0) * (size_t)WW;
	int32_t present = 0, gains = 0, losses = 0; // a chunk has at most 2^24 items
	for (int32_t w = lane; w < WW; w += WAVE) {
		const unsigned long long s = row[w], p = up >= 0 ? prow[w] : s;
		present += __popcll(s), gains += __popcll(s & ~p), losses += __popcll(~s & p);
	}
	for (int32_t d = WAVE / 2; d > 0; d >>= 1) present += __shfl_down(present, d), gains += __shfl_down(gains, d), losses += __shfl_down(losses, d);
	if (lane == 0) {
		long long *o = node + (size_t)k * 3;
		o[0] += present, o[1] += gains, o[2] += losses;
	}
}
