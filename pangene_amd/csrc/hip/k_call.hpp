// ------------------------------------------------------------------------------------------------
// pangene.js call, the walk side (pangene.js:812-862): which walks pass through which bubble, the alleles they take and the genes
// inside.  The script keeps, per end vertex, the starts seen so far in the current walk and never clears them when an end closes;
// as a set its records are: for every (bubble, orientation) with start u and end v, one record per pair p < i of positions of ONE
// walk with walk[p] == u and walk[i] == v.  That closed form is what runs here:
//   keys     (walk, vertex) -> position, sorted (stable: positions ascend inside a key) -- the per-walk index
//   count    per position i: over the (bubble, orientation)s ending at walk[i], the earlier occurrences of their start (two binary
//            searches each), then a scan and
//   emit     the records, in (position, bubble, st_off, orientation) order; a stable sort by bubble gives the script's order
//            (bubble, walk, en_off, st_off, orientation).
// Alleles: a hash of every record's oriented path, records sorted by (bubble, hash) (stable: record order inside), and every record
// compared element by element with the first of its run -- and, when that differs (a collision), with the records before it in the
// run -- so that a collision never merges two alleles.  Genes: every interior step as (bubble, segment) -> its position in record
// order, sorted; the first of each key is the gene's first appearance.
// Tested directly, without a graph: tests/support/call_direct.py gives pga_call_bubbles walks and bubbles no GFA has (hairpins, shared
// end vertices, empty walks, R > N and I > R, few hash bits) and compares every output array with the plain restatement of the
// contract in tests/support/call_ref.py.
// ------------------------------------------------------------------------------------------------

__device__ __forceinline__ int64_t call_lower_u64(const uint64_t *a, int64_t lo, int64_t hi, uint64_t x)
{
	while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (a[m] < x) lo = m + 1; else hi = m; }
	return lo;
}
__device__ __forceinline__ int64_t call_lower_u32(const uint32_t *a, int64_t lo, int64_t hi, uint32_t x)
{
	while (lo < hi) { const int64_t m = (lo + hi) >> 1; if (a[m] < x) lo = m + 1; else hi = m; }
	return lo;
}

// per position: its walk, and the key (walk, vertex) of the per-walk index
__global__ __launch_bounds__(BLOCK) void k_call_keys(const int32_t *step, const int64_t *woff, int32_t n_walk, int64_t n, int vb,
                                                      int32_t *wid, uint64_t *key, uint32_t *val)
{
	const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (g >= n) return;
	int32_t lo = 0, hi = n_walk; // last walk that starts at or before g (empty walks share their offset with the next one)
	while (hi - lo > 1) { const int32_t m = (lo + hi) >> 1; if (woff[m] <= g) lo = m; else hi = m; }
	wid[g] = lo;
	key[g] = (uint64_t)lo << vb | (uint32_t)step[g];
	val[g] = (uint32_t)g;
}

struct CallIdx { // the sorted per-walk index and the (bubble, orientation)s by end vertex
	const uint64_t *key; const uint32_t *pos; int64_t n; int vb;
	const int32_t *eoff, *ebo, *est; // entries ending at vertex x: [eoff[x], eoff[x+1]), bubble*2+ori and start vertex, by bo
};

// earlier occurrences of vertex u in walk w before position g: [*lo, *lo + return)
__device__ __forceinline__ int32_t call_before(const CallIdx &ix, int32_t w, int32_t u, int64_t g, int64_t *lo)
{
	const uint64_t k = (uint64_t)w << ix.vb | (uint32_t)u;
	const int64_t a = call_lower_u64(ix.key, 0, ix.n, k), b = call_lower_u64(ix.key, a, ix.n, k + 1);
	*lo = a;
	return (int32_t)(call_lower_u32(ix.pos, a, b, (uint32_t)g) - a);
}

__global__ __launch_bounds__(BLOCK) void k_call_count(CallIdx ix, const int32_t *step, const int32_t *wid, int32_t *cnt)
{
	const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (g >= ix.n) return;
	const int32_t x = step[g], w = wid[g];
	int32_t c = 0;
	int64_t lo;
	for (int32_t e = ix.eoff[x]; e < ix.eoff[x + 1]; ++e) c += call_before(ix, w, ix.est[e], g, &lo);
	cnt[g] = c;
}

__global__ __launch_bounds__(BLOCK) void k_call_emit(CallIdx ix, const int32_t *step, const int32_t *wid, const int64_t *woff, const int32_t *off, int4 *rec)
{
	const int64_t g = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (g >= ix.n) return;
	const int32_t x = step[g], w = wid[g];
	const int64_t w0 = woff[w];
	int64_t o = off[g];
	for (int32_t e = ix.eoff[x]; e < ix.eoff[x + 1]; ++e) {
		int64_t a, b = 0;
		const int32_t na = call_before(ix, w, ix.est[e], g, &a);
		int32_t nb = 0;
		const bool two = e + 1 < ix.eoff[x + 1] && (ix.ebo[e + 1] >> 1) == (ix.ebo[e] >> 1); // both orientations end here: merge by st_off
		if (two) nb = call_before(ix, w, ix.est[e + 1], g, &b);
		for (int32_t i = 0, j = 0; i < na || j < nb;) {
			const bool first = j >= nb || (i < na && ix.pos[a + i] <= ix.pos[b + j]);
			const uint32_t p = first ? ix.pos[a + i++] : ix.pos[b + j++];
			rec[o++] = make_int4(first ? ix.ebo[e] : ix.ebo[e + 1], w, (int32_t)(p - w0), (int32_t)(g - w0));
		}
		if (two) ++e;
	}
}

__global__ __launch_bounds__(BLOCK) void k_call_bub_keys(const int4 *rec, int64_t n, uint64_t *key, uint32_t *val)
{
	const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (r >= n) return;
	key[r] = (uint64_t)(rec[r].x >> 1);
	val[r] = (uint32_t)r;
}

__global__ __launch_bounds__(BLOCK) void k_call_gather(const int4 *in, const uint32_t *idx, int64_t n, int4 *out)
{
	const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (r < n) out[r] = in[idx[r]];
}

// the k-th vertex of a record's oriented path (start to end of the bubble)
__device__ __forceinline__ int32_t call_path_at(const int4 r, const int32_t *step, const int64_t *woff, int32_t k)
{
	const int32_t *w = step + woff[r.y];
	return (r.x & 1) == 0 ? w[r.z + k] : (w[r.w - k] ^ 1);
}
__device__ bool call_same_path(const int4 a, const int4 b, const int32_t *step, const int64_t *woff)
{
	if (a.w - a.z != b.w - b.z) return false;
	for (int32_t k = 0; k <= a.w - a.z; ++k)
		if (call_path_at(a, step, woff, k) != call_path_at(b, step, woff, k)) return false;
	return true;
}

// (bubble, hash of the oriented path) per record; hb = bits of the hash kept (PANGENE_CALL_HASH_BITS makes collisions likely)
__global__ __launch_bounds__(BLOCK) void k_call_hash(const int4 *rec, int64_t n, const int32_t *step, const int64_t *woff, int hb,
                                                      uint64_t *key, uint32_t *val, int32_t *n_int)
{
	const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (r >= n) return;
	const int4 x = rec[r];
	uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)(x.w - x.z);
	for (int32_t k = 0; k <= x.w - x.z; ++k) {
		h = (h ^ (uint32_t)call_path_at(x, step, woff, k)) * 0xff51afd7ed558ccdull;
		h ^= h >> 31;
	}
	h ^= h >> 29;
	key[r] = (uint64_t)(x.x >> 1) << hb | (h >> (64 - hb));
	val[r] = (uint32_t)r;
	n_int[r] = x.w - x.z - 1 > 0 ? x.w - x.z - 1 : 0;
}

struct CallRunHead { const uint64_t *k; __device__ __forceinline__ I32 operator()(int64_t i) const { return I32{(i == 0 || k[i] != k[i - 1]) ? (int32_t)i : 0}; } };

// rep[r] = the first record of r's run with the same path; cnt[rep] = records of the allele
__global__ __launch_bounds__(BLOCK) void k_call_rep(const int4 *rec, const uint32_t *val, const int32_t *run, int64_t n, const int32_t *step,
                                                     const int64_t *woff, int32_t *rep, int32_t *cnt)
{
	const int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (j >= n) return;
	const uint32_t r = val[j];
	const int64_t s = run[j];
	uint32_t f = r;
	if (s < j) {
		const int4 x = rec[r];
		for (int64_t t = s; t < j; ++t) // the head first; the rest only after a collision
			if (call_same_path(rec[val[t]], x, step, woff)) { f = val[t]; break; }
	}
	rep[r] = (int32_t)f;
	atomicAdd(&cnt[f], 1);
}

// every interior step as (bubble * n_seg + segment) -> its number in record order
__global__ __launch_bounds__(BLOCK) void k_call_interior(const int4 *rec, int64_t n, const int32_t *ioff, const int32_t *step, const int64_t *woff,
                                                          int64_t n_seg, uint64_t *key, uint32_t *val)
{
	const int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (r >= n) return;
	const int4 x = rec[r];
	const int32_t *w = step + woff[x.y];
	const uint64_t base = (uint64_t)(x.x >> 1) * (uint64_t)n_seg;
	int64_t o = ioff[r];
	for (int32_t k = x.z + 1; k < x.w; ++k, ++o) key[o] = base + (uint64_t)(w[k] >> 1), val[o] = (uint32_t)o;
}

struct CallKeyHead { const uint64_t *k; __device__ __forceinline__ I32 operator()(int64_t i) const { return I32{(i == 0 || k[i] != k[i - 1]) ? 1 : 0}; } };

__global__ __launch_bounds__(BLOCK) void k_call_genes(const uint64_t *key, const uint32_t *val, int64_t n, const int32_t *hoff, int64_t n_seg,
                                                       int32_t *gbub, int32_t *gseg, uint32_t *gfirst)
{
	const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n || (i > 0 && key[i] == key[i - 1])) return;
	const int64_t h = hoff[i];
	gbub[h] = (int32_t)(key[i] / (uint64_t)n_seg), gseg[h] = (int32_t)(key[i] % (uint64_t)n_seg), gfirst[h] = val[i];
}
