// ------------------------------------------------------------------------------------------------
// Gain and loss rates on a tree (pga_pan_rates, include/pangene_hip.h; DESIGN.md section 8 "Gain and loss rates"): the two-state Markov
// model per item over the postfix program k_gainloss runs, in fp64, one lane per item, uniform control flow.  The device sees tables
// only: tab[set][k][4] = P00 P01 P10 P11 of the branch above the node of op k, pi[set][2]; nothing here takes an exponential, a
// logarithm or divides by a rate.
//   k_rt_up    the program forwards, grid.y = the parameter set.  The node of op k has in_k = (in0, in1), the likelihood of the leaves
//              below it given its state, and an exponent E: the true value is in_k 2^E.  After every join both values are divided by
//              2^e, e the binary exponent of the larger one (rt_exponent / rt_scale: integer operations on the high word, exact), and
//              E += e, so no value ever leaves fp64's range.  What goes on the stack is not in_k but what the parent multiplies:
//              m_k(a) = P_a0 in_k(0) + P_a1 in_k(1) with the table row of op k -- a wave-uniform load, the next row fetched while this
//              one is used.  The top entry (m0, m1, E) lives in registers, the ones below in LDS, lane-interleaved.  With rows != nullptr
//              set 0 stores the scaled in_k of every op, 16 bytes a lane.  lik_m 2^lik_e = pi0 in_root(0) + pi1 in_root(1).
//   k_rt_down  set 0, the program backwards.  The stack holds out_v, the outside vector over the own state of a join whose children are
//              still to come (power-of-two scaled: only ratios are read); a join is stored once, its later child reads it and its
//              earlier child takes it off.  Visiting op k with parent v and sibling d:
//              O(a) = out_v(a) m_d(a), J(a, b) = O(a) P^k_ab in_k(b), out_k(b) = O(0) P^k_0b + O(1) P^k_1b, Z = sum J;
//              present = (J01 + J11) / Z, gain = J01 / Z, loss = J10 / Z.  The lane adds gain and loss to its item's totals, the wave's
//              three sums go to part[k][wave][3] through a fixed __shfl_down tree.
//   k_rt_node  per op the partials in ascending wave order, added into node[k][3]: a plain load, add and store, the launches of a call
//              follow each other on one stream.
// Lanes past the chunk run its last item again and store nothing.
// ------------------------------------------------------------------------------------------------
constexpr int32_t RT_BLOCK = 128;      // lanes (items) of a workgroup of k_rt_up / k_rt_down: two waves
constexpr int32_t RT_DEPTH = 16;       // stack entries a program may need
constexpr int32_t RT_MAX_SET = 64;
constexpr int32_t RT_NODE_BLOCK = 256; // k_rt_node: four waves, four ops
constexpr int32_t RT_AHEAD = 4;        // k_rt_down: ops whose rows are loaded ahead

// frexp's exponent of x >= 0: x = m 2^e with m in [0.5, 1).  0 for zero, a subnormal, an infinity or a NaN, which are left as they are.
__device__ __forceinline__ int32_t rt_exponent(double x)
{
	const int32_t b = (__double2hiint(x) >> 20) & 0x7ff;
	return b == 0 || b == 0x7ff ? 0 : b - 1022;
}
// ldexp(x, -e) for x >= 0 by the high word; zero stays zero, and what would leave the normal range below becomes zero
__device__ __forceinline__ double rt_scale(double x, int32_t e)
{
	const int32_t hi = __double2hiint(x), b = (hi >> 20) & 0x7ff;
	if (b == 0 || b == 0x7ff) return b == 0 ? 0.0 : x;
	if (b - e <= 0) return 0.0;
	return __hiloint2double(hi - e * (1 << 20), __double2loint(x));
}

// grid: (ceil(Gc / 128), n_set).  ops[ceil(n_op / 32)], bits[n_leaf][W] of ALL items (the chunk starts at item g0 and has Gc items),
// tab[n_set][n_op][4], pi[n_set][2], lik_m / lik_e[n_set][G], rows: nullptr or [n_op][Gc] double2.
// dynamic LDS: max(depth - 1, 1) * RT_BLOCK * (2 doubles + 1 int32)
__global__ __launch_bounds__(RT_BLOCK) void k_rt_up(const uint32_t *__restrict__ ops, const uint32_t *__restrict__ bits, int32_t g0, int32_t Gc, int32_t G, int32_t W,
                                                     int32_t n_leaf, int32_t n_op, int32_t n_slot, const double *__restrict__ tab, const double *__restrict__ pi,
                                                     double *__restrict__ lik_m, int32_t *__restrict__ lik_e, double2 *__restrict__ rows)
{
	extern __shared__ double rt_stack[];
	int32_t *rt_exp = (int32_t *)(rt_stack + (size_t)n_slot * 2 * RT_BLOCK);
	const int32_t l = (int32_t)threadIdx.x, set = (int32_t)blockIdx.y;
	const int32_t c = (int32_t)blockIdx.x * RT_BLOCK + l; // the item inside the chunk
	const bool mine = c < Gc;
	const int32_t g = g0 + min(c, Gc - 1);
	const uint32_t *my_bits = bits + (size_t)(g >> 5);
	const double *my_tab = tab + (size_t)set * (size_t)n_op * 4;
	const bool keep = rows != nullptr && set == 0 && mine;

	double t0 = 0, t1 = 0;    // the top entry
	int32_t tE = 0;
	int32_t sp = 0, leaf = 0; // entries on the stack, leaves pushed: both wave-uniform
	uint32_t op_word = 0, gene_word = 0;
	double n00 = my_tab[0], n01 = my_tab[1], n10 = my_tab[2], n11 = my_tab[3]; // the row of the next op
	for (int32_t k = 0; k < n_op; ++k) {
		const double p00 = n00, p01 = n01, p10 = n10, p11 = n11;
		{
			const double *nx = my_tab + (size_t)min(k + 1, n_op - 1) * 4;
			n00 = nx[0], n01 = nx[1], n10 = nx[2], n11 = nx[3];
		}
		if ((k & 31) == 0) op_word = ops[k >> 5];
		double i0, i1;
		int32_t E;
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
				double *e = rt_stack + (size_t)(sp - 1) * 2 * RT_BLOCK + l;
				e[0] = t0, e[RT_BLOCK] = t1, rt_exp[(sp - 1) * RT_BLOCK + l] = tE;
			}
			const bool b = (gene_word >> (leaf & 31)) & 1u;
			i0 = b ? 0.0 : 1.0, i1 = b ? 1.0 : 0.0, E = 0;
			++sp, ++leaf;
		} else { // join the entry below the top with the top
			const double *e = rt_stack + (size_t)(sp - 2) * 2 * RT_BLOCK + l;
			i0 = e[0] * t0, i1 = e[RT_BLOCK] * t1;
			const int32_t ex = rt_exponent(fmax(i0, i1));
			i0 = rt_scale(i0, ex), i1 = rt_scale(i1, ex);
			E = rt_exp[(sp - 2) * RT_BLOCK + l] + tE + ex;
			--sp;
		}
		if (keep) rows[(size_t)k * (size_t)Gc + (size_t)c] = make_double2(i0, i1);
		if (k < n_op - 1) t0 = p00 * i0 + p01 * i1, t1 = p10 * i0 + p11 * i1;
		else t0 = i0, t1 = i1; // the root has no branch above it
		tE = E;
	}
	if (mine) {
		const double L = pi[2 * set] * t0 + pi[2 * set + 1] * t1;
		const int32_t ex = rt_exponent(L);
		const double m = rt_scale(L, ex);
		lik_m[(size_t)set * (size_t)G + (size_t)g] = m;
		lik_e[(size_t)set * (size_t)G + (size_t)g] = m > 0.0 ? tE + ex : 0;
	}
}

// grid: ceil(Gc / 128).  sib[n_op] = the op of the sibling, -1 for the root; tab, pi of set 0; rows[n_op][Gc]; n_sum: the items
// [0, n_sum) count for part[n_op][WC][3], WC = ceil(Gc / 64); gene[G][3]; pres: nullptr or [n_op][Gc].
// dynamic LDS: max(depth - 1, 1) * RT_BLOCK * 2 doubles
__global__ __launch_bounds__(RT_BLOCK) void k_rt_down(const uint32_t *__restrict__ ops, const int32_t *__restrict__ sib, int32_t g0, int32_t Gc, int32_t n_op, int32_t n_sum,
                                                       int32_t WC, const double *__restrict__ tab, const double *__restrict__ pi, const double2 *__restrict__ rows,
                                                       double *__restrict__ part, double *__restrict__ gene, double *__restrict__ pres)
{
	extern __shared__ double rt_stack[];
	const int32_t l = (int32_t)threadIdx.x;
	const int32_t c = (int32_t)blockIdx.x * RT_BLOCK + l;
	const bool mine = c < Gc;
	const int32_t cc = min(c, Gc - 1);
	const bool counts = mine && g0 + c < n_sum;
	const int32_t wave = c >> 6;
	const bool writer = (l & (WAVE - 1)) == 0 && wave < WC;
	const double pi0 = pi[0], pi1 = pi[1];

	double u0 = 0, u1 = 0; // the top entry
	int32_t n = 0;         // entries on the stack: wave-uniform
	double gains = 0, losses = 0, root = 0;
	uint32_t op_word = 0;
	for (int32_t kb = n_op - 1; kb >= 0; kb -= RT_AHEAD) {
		double2 mine_in[RT_AHEAD], sib_in[RT_AHEAD];
		int32_t sb[RT_AHEAD];
#pragma unroll
		for (int32_t j = 0; j < RT_AHEAD; ++j) {
			const int32_t k = max(kb - j, 0);
			sb[j] = sib[k];
			mine_in[j] = rows[(size_t)k * (size_t)Gc + (size_t)cc];
			sib_in[j] = rows[(size_t)max(sb[j], 0) * (size_t)Gc + (size_t)cc];
		}
#pragma unroll
		for (int32_t j = 0; j < RT_AHEAD; ++j) {
			const int32_t k = kb - j;
			if (k < 0) break;
			if (k == n_op - 1 || (k & 31) == 31) op_word = ops[k >> 5];
			const double i0 = mine_in[j].x, i1 = mine_in[j].y;
			double o0, o1, present, gain, loss;
			if (k == n_op - 1) { // the root
				const double z0 = pi0 * i0, z1 = pi1 * i1, Z = z0 + z1;
				present = Z > 0.0 ? z1 * (1.0 / Z) : 0.0, gain = 0.0, loss = 0.0;
				root = present;
				o0 = pi0, o1 = pi1;
			} else {
				const double *pk = tab + (size_t)k * 4, *pd = tab + (size_t)sb[j] * 4;
				const double d0 = sib_in[j].x, d1 = sib_in[j].y;
				const double O0 = u0 * (pd[0] * d0 + pd[1] * d1), O1 = u1 * (pd[2] * d0 + pd[3] * d1);
				const double J00 = O0 * pk[0] * i0, J01 = O0 * pk[1] * i1, J10 = O1 * pk[2] * i0, J11 = O1 * pk[3] * i1;
				const double Z = (J00 + J01) + (J10 + J11);
				const double r = Z > 0.0 ? 1.0 / Z : 0.0;
				present = (J01 + J11) * r, gain = J01 * r, loss = J10 * r;
				o0 = O0 * pk[0] + O1 * pk[2], o1 = O0 * pk[1] + O1 * pk[3];
				const int32_t ex = rt_exponent(fmax(o0, o1));
				o0 = rt_scale(o0, ex), o1 = rt_scale(o1, ex);
				gains += gain, losses += loss;
				if (sb[j] > k) { // the earlier child of its parent, visited last: the parent's entry goes
					--n;
					if (n > 0) {
						const double *e = rt_stack + (size_t)(n - 1) * 2 * RT_BLOCK + l;
						u0 = e[0], u1 = e[RT_BLOCK];
					}
				}
			}
			if (pres != nullptr && mine) pres[(size_t)k * (size_t)Gc + (size_t)c] = present;
			double s0 = counts ? present : 0.0, s1 = counts ? gain : 0.0, s2 = counts ? loss : 0.0;
			for (int32_t d = WAVE / 2; d > 0; d >>= 1) s0 += __shfl_down(s0, d), s1 += __shfl_down(s1, d), s2 += __shfl_down(s2, d);
			if (writer) {
				double *o = part + ((size_t)k * (size_t)WC + (size_t)wave) * 3;
				o[0] = s0, o[1] = s1, o[2] = s2;
			}
			if ((op_word >> (k & 31)) & 1u) { // a join: its children read this vector
				if (n > 0) {
					double *e = rt_stack + (size_t)(n - 1) * 2 * RT_BLOCK + l;
					e[0] = u0, e[RT_BLOCK] = u1;
				}
				u0 = o0, u1 = o1;
				++n;
			}
		}
	}
	if (mine) {
		double *o = gene + (size_t)(g0 + c) * 3;
		o[0] = gains, o[1] = losses, o[2] = root;
	}
}

// grid: ceil(n_op / 4).  node[n_op][3] += the chunk's partials part[n_op][WC][3], wave 0 first
__global__ __launch_bounds__(RT_NODE_BLOCK) void k_rt_node(const double *__restrict__ part, int32_t n_op, int32_t WC, double *__restrict__ node)
{
	const int32_t lane = (int32_t)threadIdx.x & (WAVE - 1);
	const int32_t k = (int32_t)blockIdx.x * (RT_NODE_BLOCK / WAVE) + ((int32_t)threadIdx.x >> 6);
	if (k >= n_op || lane >= 3) return;
	const double *p = part + (size_t)k * (size_t)WC * 3 + lane;
	double acc = 0.0;
	for (int32_t w0 = 0; w0 < WC; w0 += 8) {
		double v[8];
#pragma unroll
		for (int32_t j = 0; j < 8; ++j) v[j] = w0 + j < WC ? p[(size_t)(w0 + j) * 3] : 0.0;
#pragma unroll
		for (int32_t j = 0; j < 8; ++j) acc += v[j];
	}
	node[(size_t)k * 3 + lane] += acc;
}
