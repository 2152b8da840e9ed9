// tree.cpp -- a tree of the assemblies from their pairwise distances (pg_tree_file, pg_write_tree, pg_pan_join, pg_pan_tree;
// include/pangene_amd.h).  The distances of pangene dist become fixed-point integers, neighbour-joining or UPGMA joins them in integer
// arithmetic (DESIGN.md section 8 "Trees": every sum is an integer sum, ties go to the smallest slot numbers), and only the Newick text
// is floating point.  The joins run on the backend (pga_pan_join), or as the plain loops below when the backend has no such entry.
// Bootstrap support (pg_pan_boot, pg_pan_boot_records, pangene tree -b; DESIGN.md section 8 "Bootstrap"): the replicates' records come from
// the backend in chunks (pga_pan_boot), or from the plain loops below, and are folded into per-join counts here, in code both builds share.
// Clusters (pg_cluster_file, pg_write_cluster, pg_pan_medoids, pg_pan_cluster, pangene cluster; DESIGN.md section 8 "Clusters"): k-medoids
// over the same fixed-point distances, on the backend (pga_pan_medoids) or as the plain loops below; the silhouettes and the text are
// code both builds share.
// PERMANOVA (pg_pan_permanova, pg_pan_permanova_presence, pangene permanova; DESIGN.md section 8 "PERMANOVA"): per trait the compacted
// submatrix of the same distances, its scaling, and T, A, B of the observed labels and the permutation count k from the backend
// (pga_pan_permanova) or from the plain loops below; the statistics and the text are code both builds share.  trait.cpp reads the trait
// file and calls permanova_run.
// Mantel test (pg_mantel_file, pg_write_mantel, pg_pan_mantel, pangene mantel; DESIGN.md section 8 "Mantel test"): two fixed-point matrices
// over the same assemblies -- two of the distances above, or one of them and a matrix read from a file --, their shifts and sums, and Z of
// the identity order and the two permutation counts from the backend (pga_pan_mantel) or from the plain loops below; r, the p values and
// the text are code both builds share.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>
#include "pg_internal.hpp"

// The replicates one pan_boot call takes.  It is not in the backend table (the table's last member is pan_boot), so it is found by
// name: a library whose backend sets pan_boot exports it, a library without pan_boot (the checker build) does not, and the weak
// declaration is then null.  The two go together: boot_walk treats pan_boot without pga_boot_batch as an error, not as "no backend".
extern "C" int32_t pga_boot_batch(int32_t n_asm) __attribute__((weak));

namespace pgx {
namespace {

constexpr int64_t JOIN_IN_MAX = (int64_t)1 << 29; // an input entry stays below this in size
constexpr int64_t JOIN_MAX = (int64_t)1 << 30;    // and every distance made on the way below this

inline int64_t floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && ((a < 0) != (b < 0))) ? q - 1 : q; } // b > 0 here

// S[A][A] -> q[A][A] = distance * 2^F; 0, or PGA_ERR_RANGE when the differences leave no fraction bit
int to_fixed(const int32_t *S, int32_t A, int32_t metric, int32_t *q, int32_t *frac_bits)
{
	const size_t n = (size_t)A;
	int32_t F = 20;
	if (metric == PG_DIST_DIFF) {
		int64_t mx = 0;
		for (size_t i = 0; i < n; ++i)
			for (size_t j = 0; j < n; ++j) mx = std::max<int64_t>(mx, (int64_t)S[i * n + i] + S[j * n + j] - 2 * (int64_t)S[i * n + j]);
		int bl = 0;
		while ((mx >> bl) != 0) ++bl;
		F = std::min(20, 29 - bl);
		if (F < 0) return PGA_ERR_RANGE;
	}
	for (size_t i = 0; i < n; ++i)
		for (size_t j = 0; j < n; ++j) {
			const int64_t ni = S[i * n + i], nj = S[j * n + j], s = S[i * n + j];
			if (metric == PG_DIST_DIFF) q[i * n + j] = (int32_t)((ni + nj - 2 * s) << F);
			else {
				const int64_t u = ni + nj - s;
				q[i * n + j] = u == 0 ? 0 : (int32_t)((((int64_t)1 << 21) * (u - s) + u) / (2 * u));
			}
		}
	*frac_bits = F;
	return 0;
}

// The joins as the definition states them, slot by slot: d[n][n] in place (32-bit storage: a value that passes the range test fits),
// rec[n_rec][6].  The first distance out of range ends the run, which is what a flag read at the end amounts to.
int join_host(std::vector<int32_t> &d, int32_t n, int32_t method, int64_t *rec)
{
	const size_t N = (size_t)n;
	std::vector<int32_t> live(N), size(N, 1);
	std::vector<int64_t> R(N, 0);
	for (size_t x = 0; x < N; ++x) {
		live[x] = (int32_t)x;
		for (size_t y = 0; y < N; ++y) R[x] += d[x * N + y];
	}
	const bool nj = method == PG_TREE_NJ;
	// PANGENE_TREE_STOP_AFTER=k (timing only, tests/run_tree_timing.py): give up after k joins with status 1, so that a large input
	// can be timed on its first joins
	const char *stop_s = std::getenv("PANGENE_TREE_STOP_AFTER");
	const long stop = stop_s ? std::atol(stop_s) : 0;
	long done = 0;
	while ((int32_t)live.size() > (nj ? 3 : 1)) {
		if (stop > 0 && done++ >= stop) return 1;
		const int64_t r = (int64_t)live.size();
		int64_t best = 0;
		size_t bi = 0, bj = 0;
		bool have = false;
		for (size_t a = 0; a < live.size(); ++a) {
			const size_t i = (size_t)live[a];
			const int32_t *row = d.data() + i * N;
			for (size_t b = a + 1; b < live.size(); ++b) {
				const size_t j = (size_t)live[b];
				const int64_t c = nj ? (r - 2) * (int64_t)row[j] - R[i] - R[j] : (int64_t)row[j];
				if (!have || c < best) best = c, bi = i, bj = j, have = true;
			}
		}
		const int64_t dij = d[bi * N + bj], ni = size[bi], nn = size[bj];
		rec[0] = (int64_t)bi, rec[1] = (int64_t)bj, rec[2] = dij, rec[3] = nj ? R[bi] : ni, rec[4] = nj ? R[bj] : nn, rec[5] = r;
		rec += 6;
		int64_t sum = 0;
		for (const int32_t kk : live) {
			const size_t k = (size_t)kk;
			if (k == bi || k == bj) continue;
			const int64_t a = d[bi * N + k], b = d[bj * N + k];
			const int64_t v = nj ? floor_div(a + b - dij, 2) : floor_div(ni * a + nn * b, ni + nn);
			if (v >= JOIN_MAX || v <= -JOIN_MAX) return PGA_ERR_RANGE;
			d[bi * N + k] = d[k * N + bi] = (int32_t)v;
			R[k] += v - a - b;
			sum += v;
		}
		R[bi] = sum;
		size[bi] = (int32_t)(ni + nn);
		live.erase(std::find(live.begin(), live.end(), (int32_t)bj));
	}
	if (nj) {
		const size_t x = (size_t)live[0], y = (size_t)live[1], z = (size_t)live[2];
		rec[0] = (int64_t)x, rec[1] = (int64_t)y, rec[2] = (int64_t)z, rec[3] = d[x * N + y], rec[4] = d[x * N + z], rec[5] = d[y * N + z];
	}
	return 0;
}

double t_join = 0; // seconds of the last join step (backend or host loops)

// q[n][n] (symmetric, zero diagonal, every entry below 2^29 in size), n >= 3 -> rec; 0 or a PGA_ERR_* code
int join_run(const int32_t *q, int32_t n, int32_t method, int64_t *rec)
{
	if (q == nullptr || rec == nullptr || n < 3 || (method != PG_TREE_NJ && method != PG_TREE_UPGMA)) return PGA_ERR_ARG;
	if (n > 65535) return PGA_ERR_RANGE;
	const size_t N = (size_t)n;
	for (size_t i = 0; i < N; ++i) {
		if (q[i * N + i] != 0) return PGA_ERR_ARG;
		for (size_t j = i + 1; j < N; ++j) {
			if (q[i * N + j] != q[j * N + i]) return PGA_ERR_ARG;
			if (q[i * N + j] >= JOIN_IN_MAX || q[i * N + j] <= -JOIN_IN_MAX) return PGA_ERR_RANGE;
		}
	}
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	int rc;
	if (be->pan_join != nullptr) {
		const pga_join_in_t in{q, n, method};
		pga_join_out_t res{};
		rc = be->pan_join(&in, &res);
		if (rc == 0) std::memcpy(rec, res.rec, sizeof(int64_t) * 6 * (size_t)res.n_rec);
	} else {
		std::vector<int32_t> d(q, q + N * N);
		rc = join_host(d, n, method, rec);
	}
	t_join = now_sec() - t0;
	return rc;
}

// Replicate b of the definition as plain loops: the draws, the resampled rows, shared_count, to_fixed, join_host.  bits[A][W]
int boot_host(const std::vector<uint32_t> &bits, int32_t M, int32_t A, int32_t metric, int32_t method, uint32_t seed, uint32_t b, int64_t *rec)
{
	const size_t W = ((size_t)M + 31) / 32, nn = (size_t)A * (size_t)A;
	std::vector<uint32_t> rows((size_t)A * W, 0);
	const uint64_t x0 = mix64((uint64_t)seed << 32 | (uint64_t)b);
	for (int32_t t = 0; t < M; ++t) {
		const uint64_t m = mix64(x0 + (uint64_t)(t + 1) * 0x9E3779B97F4A7C15ull) % (uint64_t)M;
		for (size_t a = 0; a < (size_t)A; ++a)
			if (bits[a * W + (size_t)(m >> 5)] >> (m & 31) & 1u) rows[a * W + (size_t)(t >> 5)] |= 1u << (t & 31);
	}
	std::vector<int32_t> S(nn), q(nn);
	int rc = shared_count(rows, M, A, S.data());
	if (rc != 0) return rc;
	int32_t F;
	if ((rc = to_fixed(S.data(), A, metric, q.data(), &F)) != 0) return rc;
	return join_host(q, A, method, rec);
}

// The records of replicates first .. first + n - 1, chunk by chunk: use(records of the chunk [k][n_rec][6], k) after each.  The backend's
// chunk is pga_boot_batch(A) replicates, the host loops' one; host memory is bounded by a chunk.  A >= 3
template <class Use>
int boot_walk(const std::vector<uint32_t> &bits, int32_t M, int32_t A, int32_t metric, int32_t method, uint32_t seed, int32_t first, int32_t n, Use use)
{
	if (A > 65535) return PGA_ERR_RANGE;
	const pga_backend_t *be = backend_default();
	const size_t n_rec = (size_t)(method == PG_TREE_NJ ? A - 2 : A - 1);
	if (be->pan_boot != nullptr) {
		if (pga_boot_batch == nullptr) { std::fprintf(stderr, "[E::pg_pan_boot] the backend has pan_boot, but the library exports no pga_boot_batch\n"); return PGA_ERR_ARG; }
		const int32_t batch = std::max(1, pga_boot_batch(A));
		for (int32_t k = 0; k < n; k += batch) {
			const pga_boot_in_t in{bits.data(), M, A, metric, method, seed, first + k, std::min(batch, n - k), nullptr};
			pga_boot_out_t res{};
			const int rc = be->pan_boot(&in, &res);
			if (rc != 0) return rc;
			use(res.rec, in.n_rep);
		}
		return 0;
	}
	std::vector<int64_t> rec(6 * n_rec);
	for (int32_t k = 0; k < n; ++k) {
		const int rc = boot_host(bits, M, A, metric, method, seed, (uint32_t)(first + k), rec.data());
		if (rc != 0) return rc == 1 ? PGA_ERR_ARG : rc; // (1: PANGENE_TREE_STOP_AFTER, which is for timing a single tree)
		use(rec.data(), 1);
	}
	return 0;
}

// Support of the reference tree's joins among the replicates, by exact comparison of leaf sets.  The reference's leaves are numbered in
// the order its own subtrees list them (Day's numbering), so that the leaves below each of its joins are an interval [lo, hi]; a set of
// a replicate is the same set exactly when its smallest and its largest number span as many numbers as it has leaves and that interval
// is one of the reference's.  NJ compares splits of the unrooted tree, each by its side without the last-numbered leaf: for the
// reference that side is [lo, hi] or [0, lo - 1]; for a replicate's join that holds the leaf it is everything else, collected on
// the way down from the trifurcation to that leaf.  O(A) a replicate.
struct Support {
	struct Span { int32_t lo, hi, sz; };
	static Span both(const Span &a, const Span &b) { return Span{std::min(a.lo, b.lo), std::max(a.hi, b.hi), a.sz + b.sz}; }
	int32_t A, n_lab; // n_lab: the joins that can be supported: A - 3 (NJ), A - 2 (UPGMA)
	bool nj;
	int32_t last_leaf = 0;                          // the leaf numbered A - 1
	std::vector<int32_t> pos;                       // leaf -> its number
	std::unordered_map<uint64_t, int32_t> join_of;  // lo << 32 | hi -> join of the reference
	// of the replicate being folded; nodes: leaf x = x, join t = A + t
	std::vector<Span> span;
	std::vector<int32_t> at, up, kid, chain, seen;  // node at a slot; parent; the two children of a join; seen[s] = the last replicate that supported s
	int32_t n_seen = 0;

	Support(const int64_t *rec, int32_t A_, int32_t method)
	    : A(A_), n_lab(std::max(method == PG_TREE_NJ ? A_ - 3 : A_ - 2, 0)), nj(method == PG_TREE_NJ), pos((size_t)A_), span((size_t)A_ + (size_t)n_lab), at((size_t)A_),
	      up((size_t)A_ + (size_t)n_lab), kid(2 * (size_t)n_lab), seen((size_t)n_lab, 0)
	{
		const size_t n = (size_t)A;
		std::vector<int32_t> head(n), tail(n), next(n, -1), cnt(n, 1), first((size_t)n_lab), last((size_t)n_lab), size_of((size_t)n_lab);
		for (size_t x = 0; x < n; ++x) head[x] = tail[x] = (int32_t)x;
		const int32_t n_join = nj ? A - 3 : A - 1;
		for (int32_t s = 0; s < n_join; ++s) { // the leaves below slot i, then those below slot j
			const size_t i = (size_t)rec[6 * (size_t)s], j = (size_t)rec[6 * (size_t)s + 1];
			next[(size_t)tail[i]] = head[j], tail[i] = tail[j], cnt[i] += cnt[j];
			if (s < n_lab) first[(size_t)s] = head[i], last[(size_t)s] = tail[i], size_of[(size_t)s] = cnt[i];
		}
		const size_t root = (size_t)rec[6 * (size_t)(nj ? n_join : n_join - 1)];
		if (nj) { // the three subtrees of the closing record, one after the other
			const size_t y = (size_t)rec[6 * (size_t)n_join + 1], z = (size_t)rec[6 * (size_t)n_join + 2];
			next[(size_t)tail[root]] = head[y], next[(size_t)tail[y]] = head[z];
		}
		int32_t k = 0;
		for (int32_t x = head[root]; x >= 0; x = next[(size_t)x]) last_leaf = x, pos[(size_t)x] = k++;
		for (int32_t s = 0; s < n_lab; ++s) {
			int32_t l = pos[(size_t)first[(size_t)s]], h = pos[(size_t)last[(size_t)s]]; // (h - l + 1 = size_of[s])
			if (nj && h == A - 1) h = l - 1, l = 0;
			join_of.emplace((uint64_t)(uint32_t)l << 32 | (uint32_t)h, s);
		}
	}
	void hit(const Span &c, int32_t *count)
	{
		if (c.hi - c.lo + 1 != c.sz) return;
		const auto it = join_of.find((uint64_t)(uint32_t)c.lo << 32 | (uint32_t)c.hi);
		if (it != join_of.end() && seen[(size_t)it->second] != n_seen) seen[(size_t)it->second] = n_seen, ++count[(size_t)it->second];
	}
	// one replicate's records -> count[s] += 1 for every supported s
	void fold(const int64_t *rec, int32_t *count)
	{
		++n_seen;
		for (int32_t x = 0; x < A; ++x) span[(size_t)x] = Span{pos[(size_t)x], pos[(size_t)x], 1}, at[(size_t)x] = x;
		for (int32_t t = 0; t < n_lab; ++t) {
			const size_t i = (size_t)rec[6 * (size_t)t], j = (size_t)rec[6 * (size_t)t + 1];
			const int32_t v = A + t;
			span[(size_t)v] = both(span[(size_t)at[i]], span[(size_t)at[j]]);
			kid[2 * (size_t)t] = at[i], kid[2 * (size_t)t + 1] = at[j];
			up[(size_t)at[i]] = up[(size_t)at[j]] = v;
			at[i] = v;
			if (!nj || span[(size_t)v].hi != A - 1) hit(span[(size_t)v], count);
		}
		if (!nj) return;
		// the joins that hold the last leaf: from the trifurcation down to it, each against everything that is not below it
		const int64_t *fin = rec + 6 * (size_t)n_lab;
		const int32_t top[3] = {at[(size_t)fin[0]], at[(size_t)fin[1]], at[(size_t)fin[2]]};
		for (const int32_t v : top) up[(size_t)v] = -1;
		chain.clear();
		for (int32_t v = last_leaf; v >= 0; v = up[(size_t)v]) chain.push_back(v);
		Span rest{A, -1, 0};
		for (const int32_t v : top)
			if (v != chain.back()) rest = both(rest, span[(size_t)v]);
		for (size_t m = chain.size() - 1; m >= 1; --m) {
			const int32_t v = chain[m], c = chain[m - 1]; // v is a join, c its child on the way
			hit(rest, count);
			const int32_t *kd = kid.data() + 2 * (size_t)(v - A);
			rest = both(rest, span[(size_t)(kd[0] == c ? kd[1] : kd[0])]);
		}
	}
};

// count[n_rec] of the reference records rec over replicates 1 .. B; A >= 3
int boot_support(const std::vector<uint32_t> &bits, int32_t M, int32_t A, int32_t metric, int32_t method, int32_t B, uint32_t seed, const int64_t *rec, int32_t *count)
{
	const int32_t n_rec = method == PG_TREE_NJ ? A - 2 : A - 1;
	std::fill(count, count + n_rec, 0);
	count[n_rec - 1] = B; // NJ's closing record, UPGMA's root: by definition
	if (B == 0 || n_rec < 2) return 0; // A < 4 (NJ): no join that can be supported, and no device work
	Support sup(rec, A, method);
	const size_t stride = 6 * (size_t)n_rec;
	return boot_walk(bits, M, A, metric, method, seed, 1, B, [&](const int64_t *r, int32_t k) {
		for (int32_t x = 0; x < k; ++x) sup.fold(r + stride * (size_t)x, count);
	});
}

std::string quoted(const std::string &s)
{
	if (s.find_first_of("(),:;[]' \t\n") == std::string::npos) return s;
	std::string o = "'";
	for (const char c : s) { o += c; if (c == '\'') o += c; }
	return o + "'";
}

std::string len_text(double fixed, int32_t F)
{
	char b[64];
	std::snprintf(b, sizeof(b), ":%.6f", fixed / (double)((int64_t)1 << F));
	return b;
}

// "P" behind the node of a join: count of B replicates in per cent, rounded half up; nothing without a bootstrap
std::string support_text(const int32_t *count, size_t s, int32_t B)
{
	return B > 0 ? std::to_string((200 * (int64_t)count[s] + B) / (2 * (int64_t)B)) : std::string();
}

// the records of n >= 3 leaves -> one Newick line; B > 0: count[] labels the joins' nodes
std::string newick(const std::vector<std::string> &names, const int64_t *rec, int32_t method, int32_t F, const int32_t *count = nullptr, int32_t B = 0)
{
	const size_t n = names.size();
	std::vector<std::string> sub(n);
	std::vector<double> height(n, 0.0);
	for (size_t i = 0; i < n; ++i) sub[i] = quoted(names[i]);
	if (method == PG_TREE_NJ) {
		for (size_t s = 0; s + 3 < n; ++s, rec += 6) {
			const size_t i = (size_t)rec[0], j = (size_t)rec[1];
			const double li = ((double)rec[2] + (double)(rec[3] - rec[4]) / (double)(rec[5] - 2)) / 2.0, lj = (double)rec[2] - li;
			sub[i] = "(" + sub[i] + len_text(li, F) + "," + sub[j] + len_text(lj, F) + ")" + support_text(count, s, B);
			std::string().swap(sub[j]);
		}
		const size_t x = (size_t)rec[0], y = (size_t)rec[1], z = (size_t)rec[2];
		const double lx = (double)(rec[3] + rec[4] - rec[5]) / 2.0, ly = (double)(rec[3] + rec[5] - rec[4]) / 2.0, lz = (double)(rec[4] + rec[5] - rec[3]) / 2.0;
		return "(" + sub[x] + len_text(lx, F) + "," + sub[y] + len_text(ly, F) + "," + sub[z] + len_text(lz, F) + ");\n";
	}
	size_t root = 0;
	for (size_t s = 0; s + 1 < n; ++s, rec += 6) {
		const size_t i = (size_t)rec[0], j = (size_t)rec[1];
		const double h = (double)rec[2] / 2.0;
		sub[i] = "(" + sub[i] + len_text(h - height[i], F) + "," + sub[j] + len_text(h - height[j], F) + ")" + (s + 2 < n ? support_text(count, s, B) : std::string());
		std::string().swap(sub[j]);
		height[i] = h, root = i;
	}
	return sub[root] + ";\n";
}

// PANGENE_TREE_TIMING=1: one line on stderr per call
void report_time(const char *route, int32_t M, int32_t A, double t_prep, double t_write)
{
	if (std::getenv("PANGENE_TREE_TIMING") == nullptr) return;
	std::fprintf(stderr, "[tree-timing] route=%s items=%d assemblies=%d prep_ms=%.3f join_ms=%.3f write_ms=%.3f\n", route, M, A, t_prep * 1e3,
	             t_join * 1e3, t_write * 1e3);
}

// bit rows -> S -> q -> rec; A >= 3
int tree_records(const std::vector<uint32_t> &bits, int32_t M, int32_t A, int32_t metric, int32_t method, std::vector<int32_t> &q, int64_t *rec, int32_t *F)
{
	const size_t nn = (size_t)A * (size_t)A;
	std::vector<int32_t> S(nn);
	int rc = shared_count(bits, M, A, S.data());
	if (rc != 0) return rc;
	q.resize(nn);
	if ((rc = to_fixed(S.data(), A, metric, q.data(), F)) != 0) return rc;
	return A >= 3 ? join_run(q.data(), A, method, rec) : 0;
}

int tree_run(const char *route, const std::vector<std::string> &names, const std::vector<uint32_t> &bits, int32_t M, const pg_tree_opt_t *o, double t_start)
{
	if ((o->metric != PG_DIST_JACCARD && o->metric != PG_DIST_DIFF) || (o->method != PG_TREE_NJ && o->method != PG_TREE_UPGMA) || o->n_boot < 0) return PGA_ERR_ARG;
	const int32_t A = (int32_t)names.size();
	const double t_prep = now_sec() - t_start;
	std::vector<int32_t> q;
	std::vector<int64_t> rec((size_t)6 * (size_t)std::max(A, 1));
	int32_t F = 20;
	t_join = 0;
	if (A >= 2) {
		const int rc = tree_records(bits, M, A, o->metric, o->method, q, rec.data(), &F);
		if (rc != 0) return rc;
	}
	std::vector<int32_t> count((size_t)std::max(A, 1), 0);
	if (A >= 3 && o->n_boot > 0) {
		const double t0 = now_sec();
		const int rc = boot_support(bits, M, A, o->metric, o->method, o->n_boot, o->seed, rec.data(), count.data());
		if (rc != 0) return rc;
		t_join += now_sec() - t0;
	}
	const double t1 = now_sec();
	OutBuf ob;
	std::string &s = ob.s;
	if (A == 0) s = ";\n";
	else if (A == 1) s = "(" + quoted(names[0]) + ");\n";
	else if (A == 2) {
		const std::string h = len_text((double)q[1] / 2.0, F);
		s = "(" + quoted(names[0]) + h + "," + quoted(names[1]) + h + ");\n";
	} else s = newick(names, rec.data(), o->method, F, count.data(), o->n_boot);
	ob.finish();
	report_time(route, M, A, t_prep, now_sec() - t1);
	return 0;
}

// ---- clusters -------------------------------------------------------------------------------------------------------------------

constexpr int32_t MED_IN_MAX = 1 << 29, MED_MAX_K = 1024;

struct Medoids { // what one run of k-medoids leaves (include/pangene_hip.h pga_medoids_out_t)
	std::vector<int32_t> medoid, label, dist, size;
	std::vector<int64_t> sums, rec;
	int64_t td = 0;
	int32_t n_swap = 0, converged = 0;
};

// k-medoids as the definition states it.  A delta is the difference of two TDs, each column's share formed directly: the column's distance
// after the exchange -- the smaller of d and its distance to the nearest medoid that stays -- minus its distance before.
void medoids_host(const int32_t *q, int32_t n, int32_t k, int32_t max_iter, Medoids &r)
{
	const size_t N = (size_t)n, K = (size_t)k;
	std::vector<int32_t> med, D(N, MED_IN_MAX), DS(N), NN(N);
	std::vector<uint8_t> in(N, 0);
	r.rec.clear();
	for (size_t s = 0; s < K; ++s) { // BUILD
		int64_t best = -1;
		size_t bx = 0;
		for (size_t x = 0; x < N; ++x) {
			if (in[x]) continue;
			int64_t g = 0;
			for (size_t o = 0; o < N; ++o) g += std::max(0, D[o] - q[x * N + o]);
			if (g > best) best = g, bx = x;
		}
		med.push_back((int32_t)bx), in[bx] = 1;
		for (size_t o = 0; o < N; ++o) D[o] = std::min(D[o], q[bx * N + o]);
		r.rec.insert(r.rec.end(), {(int64_t)bx, -1, best});
	}
	r.n_swap = 0, r.converged = 0;
	for (int32_t it = 0; it < max_iter; ++it) { // SWAP
		for (size_t o = 0; o < N; ++o) { // the nearest medoid's slot, its distance, and the distance to the nearest of the others
			int32_t d1 = MED_IN_MAX, d2 = MED_IN_MAX, nn = 0;
			for (size_t s = 0; s < K; ++s) {
				const int32_t d = q[(size_t)med[s] * N + o];
				if (d < d1) d2 = d1, d1 = d, nn = (int32_t)s;
				else if (d < d2) d2 = d;
			}
			D[o] = d1, DS[o] = d2, NN[o] = nn;
		}
		int64_t best = 0;
		size_t bx = 0, bs = 0;
		bool have = false;
		for (size_t x = 0; x < N; ++x) {
			if (in[x]) continue;
			const int32_t *row = q + x * N;
			for (size_t s = 0; s < K; ++s) {
				int64_t delta = 0;
				for (size_t o = 0; o < N; ++o) delta += std::min(row[o], NN[o] == (int32_t)s ? DS[o] : D[o]) - D[o];
				if (!have || delta < best || (delta == best && x == bx && med[s] < med[bs])) best = delta, bx = x, bs = s, have = true;
			}
		}
		if (best >= 0) { r.converged = 1; break; }
		r.rec.insert(r.rec.end(), {(int64_t)bx, (int64_t)med[bs], best});
		in[(size_t)med[bs]] = 0, in[bx] = 1, med[bs] = (int32_t)bx;
		++r.n_swap;
	}
	r.medoid = med;
	std::sort(r.medoid.begin(), r.medoid.end());
	r.label.assign(N, 0), r.dist.assign(N, 0), r.size.assign(K, 0), r.sums.assign(N * K, 0), r.td = 0;
	for (size_t c = 0; c < K; ++c) r.label[(size_t)r.medoid[c]] = -1 - (int32_t)c; // (marks the medoids)
	for (size_t o = 0; o < N; ++o) {
		if (r.label[o] < 0) r.label[o] = -1 - r.label[o];
		else {
			int32_t d = MED_IN_MAX;
			for (size_t c = 0; c < K; ++c) {
				const int32_t v = q[o * N + (size_t)r.medoid[c]];
				if (v < d) d = v, r.label[o] = (int32_t)c;
			}
			r.dist[o] = d;
		}
		++r.size[(size_t)r.label[o]], r.td += r.dist[o];
	}
	for (size_t o = 0; o < N; ++o)
		for (size_t p = 0; p < N; ++p) r.sums[o * K + (size_t)r.label[p]] += q[o * N + p];
}

double t_medoids = 0; // seconds of the k-medoids runs of the last command

// q[n][n] -> r; 0 or a PGA_ERR_* code (the table of include/pangene_hip.h pga_pan_medoids)
int medoids_run(const int32_t *q, int32_t n, int32_t k, int32_t max_iter, Medoids &r)
{
	if (q == nullptr || n < 3 || k < 2 || k > n - 1 || max_iter < 0) return PGA_ERR_ARG;
	if (n > 65535 || k > MED_MAX_K) return PGA_ERR_RANGE;
	const size_t N = (size_t)n;
	bool big = false;
	for (size_t i = 0; i < N; ++i) {
		if (q[i * N + i] != 0) return PGA_ERR_ARG;
		for (size_t j = i + 1; j < N; ++j) {
			if (q[i * N + j] != q[j * N + i] || q[i * N + j] < 0) return PGA_ERR_ARG;
			big |= q[i * N + j] >= MED_IN_MAX;
		}
	}
	if (big) return PGA_ERR_RANGE;
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	if (be->pan_medoids != nullptr) {
		const pga_medoids_in_t in{q, n, k, max_iter};
		pga_medoids_out_t res{};
		const int rc = be->pan_medoids(&in, &res);
		if (rc != 0) return rc;
		const size_t K = (size_t)k;
		r.medoid.assign(res.medoid, res.medoid + K), r.label.assign(res.label, res.label + N), r.dist.assign(res.dist, res.dist + N), r.size.assign(res.size, res.size + K);
		r.sums.assign(res.sums, res.sums + N * K), r.rec.assign(res.rec, res.rec + 3 * (size_t)res.n_rec);
		r.td = res.td, r.n_swap = res.n_swap, r.converged = res.converged;
	} else medoids_host(q, n, k, max_iter, r);
	t_medoids += now_sec() - t0;
	return 0;
}

// The silhouettes from sums and size alone.  With o in cluster c: a = sums[o][c] / (size_c - 1), b = the smallest sums[o][c'] / size_c'
// over c' != c (compared by cross-multiplication, the first of equal ones), s = (b - a) / max(a, b) as ONE division of the two
// cross-products X = sums[o][c'] (size_c - 1) and Y = sums[o][c] size_c'; 0 for a cluster of one and where both are 0.
void silhouettes(const Medoids &r, std::vector<double> &sil)
{
	const size_t N = r.label.size(), K = r.size.size();
	sil.assign(N, 0.0);
	for (size_t o = 0; o < N; ++o) {
		const size_t c = (size_t)r.label[o];
		const int64_t sc = r.size[c];
		if (sc == 1) continue;
		int64_t B = 0, sb = 0;
		for (size_t e = 0; e < K; ++e) {
			if (e == c) continue;
			const int64_t v = r.sums[o * K + e], se = r.size[e];
			if (sb == 0 || v * sb < B * se) B = v, sb = se;
		}
		const int64_t X = B * (sc - 1), Y = r.sums[o * K + c] * sb, mx = std::max(X, Y);
		if (mx != 0) sil[o] = (double)(X - Y) / (double)mx;
	}
}

// the mean over the columns of cluster c (c < 0: over all of them), summed in column order
double mean_sil(const Medoids &r, const std::vector<double> &sil, int32_t c)
{
	double s = 0;
	int64_t cnt = 0;
	for (size_t o = 0; o < sil.size(); ++o)
		if (c < 0 || r.label[o] == c) s += sil[o], ++cnt;
	return s / (double)cnt;
}

std::string fixed_text(int64_t v, int32_t F)
{
	char b[64];
	std::snprintf(b, sizeof(b), "%.6f", (double)v / (double)((int64_t)1 << F));
	return b;
}

int cluster_run(const char *route, const std::vector<std::string> &names, const std::vector<uint32_t> &bits, int32_t M, const pg_cluster_opt_t *o, double t_start)
{
	if ((o->type != PG_DIST_GENE && o->type != PG_DIST_ADJ) || (o->metric != PG_DIST_JACCARD && o->metric != PG_DIST_DIFF) || o->max_iter < 0) return PGA_ERR_ARG;
	const int32_t A = (int32_t)names.size();
	if (A < 3) { std::fprintf(stderr, "Error: pangene cluster needs at least 3 assemblies, the input has %d\n", A); return PGA_ERR_ARG; }
	if (o->k_lo < 2 || o->k_hi < o->k_lo || o->k_hi > A - 1) {
		std::fprintf(stderr, "Error: pangene cluster: k must be in [2, %d] for %d assemblies\n", A - 1, A);
		return PGA_ERR_ARG;
	}
	const double t_prep = now_sec() - t_start;
	const size_t nn = (size_t)A * (size_t)A;
	std::vector<int32_t> S(nn), q(nn);
	int rc = shared_count(bits, M, A, S.data());
	if (rc != 0) return rc;
	int32_t F = 20;
	if ((rc = to_fixed(S.data(), A, o->metric, q.data(), &F)) != 0) return rc;
	t_medoids = 0;
	OutBuf ob;
	std::string &s = ob.s;
	char b[128];
	s = "#K\tk\tTD\tmean_sil\tswaps\tconverged\n";
	Medoids best, cur;
	std::vector<double> best_sil, sil;
	double best_mean = 0;
	for (int32_t k = o->k_lo; k <= o->k_hi; ++k) {
		if ((rc = medoids_run(q.data(), A, k, o->max_iter, cur)) != 0) return rc;
		if (!cur.converged) std::fprintf(stderr, "Note: pangene cluster: k = %d did not converge within %d iterations\n", k, o->max_iter);
		silhouettes(cur, sil);
		const double mean = mean_sil(cur, sil, -1);
		std::snprintf(b, sizeof(b), "\t%.4f\t%d\t%d\n", mean, cur.n_swap, cur.converged);
		s += "K\t" + std::to_string(k) + "\t" + fixed_text(cur.td, F) + b;
		if (k == o->k_lo || mean > best_mean) best_mean = mean, std::swap(best, cur), std::swap(best_sil, sil);
	}
	const double t1 = now_sec();
	s += "#C\tcluster\tmedoid\tsize\tmean_sil\n";
	for (size_t c = 0; c < best.medoid.size(); ++c) {
		std::snprintf(b, sizeof(b), "\t%d\t%.4f\n", best.size[c], mean_sil(best, best_sil, (int32_t)c));
		s += "C\t" + std::to_string(c + 1) + "\t" + names[(size_t)best.medoid[c]] + b;
	}
	s += "#A\tassembly\tcluster\tmedoid\tdist\tsil\n";
	for (size_t x = 0; x < (size_t)A; ++x) {
		const size_t c = (size_t)best.label[x];
		std::snprintf(b, sizeof(b), "\t%.4f\n", best_sil[x]);
		s += "A\t" + names[x] + "\t" + std::to_string(c + 1) + "\t" + names[(size_t)best.medoid[c]] + "\t" + fixed_text(best.dist[x], F) + b;
		ob.flush_if_full();
	}
	ob.finish();
	if (std::getenv("PANGENE_CLUSTER_TIMING") != nullptr)
		std::fprintf(stderr, "[cluster-timing] route=%s items=%d assemblies=%d prep_ms=%.3f medoids_ms=%.3f write_ms=%.3f\n", route, M, A, t_prep * 1e3, t_medoids * 1e3,
		             (now_sec() - t1) * 1e3);
	return 0;
}

// ---- PERMANOVA ------------------------------------------------------------------------------------------------------------------

constexpr int32_t PERMA_MAX_COL = 16384, PERMA_MAX_PERM = 2147483646; // the backend's limits (include/pangene_hip.h pga_pan_permanova)

// what one trait leaves.  skip: 0 = tested, 1 = N < 3 or an empty group, 2 = every distance is zero
struct Perma { int32_t N = 0, n1 = 0, Fe = 0, skip = 1; int64_t T = 0, A = 0, B = 0, k = 0; };

typedef __int128 i128;

// The backend's step on the host, by the definition: w from qc, r and T, then per label row A as a double loop over the pairs of its
// columns and B over its columns, G in 128 bits; every permutation's row from its order by indexing.  qc[N][N], y[N]
void permanova_host(const int32_t *qc, const uint8_t *y, int32_t N, int32_t s, int32_t n1, int32_t n, uint32_t seed, Perma &r)
{
	const size_t n_ = (size_t)N;
	std::vector<int64_t> w(n_ * n_), rs(n_, 0);
	r.T = 0;
	for (size_t i = 0; i < n_; ++i)
		for (size_t j = 0; j < n_; ++j) {
			const int64_t e = i == j ? 0 : (int64_t)(qc[i * n_ + j] >> s);
			w[i * n_ + j] = e * e, rs[i] += e * e;
		}
	for (size_t i = 0; i < n_; ++i) r.T += rs[i];
	std::vector<int32_t> on;
	auto sums = [&](const uint8_t *lab, int64_t &A, int64_t &B) {
		on.clear();
		for (int32_t i = 0; i < N; ++i) if (lab[i]) on.push_back(i);
		A = B = 0;
		for (size_t a = 0; a < on.size(); ++a) {
			B += rs[(size_t)on[a]];
			for (size_t b = a + 1; b < on.size(); ++b) A += 2 * w[(size_t)on[a] * n_ + (size_t)on[b]]; // both orders of the pair
		}
	};
	auto G = [&](int64_t A, int64_t B) { return (i128)N * A - (i128)(2 * (int64_t)n1) * B; };
	sums(y, r.A, r.B);
	const i128 g_obs = G(r.A, r.B);
	std::vector<int32_t> o(n_);
	std::vector<uint8_t> yp(n_);
	r.k = 0;
	for (int32_t p = 1; p <= n; ++p) {
		fisher_yates_order(N, seed, (uint32_t)p, o.data());
		for (size_t c = 0; c < n_; ++c) yp[c] = y[(size_t)o[c]];
		int64_t A, B;
		sums(yp.data(), A, B);
		if (G(A, B) <= g_obs) ++r.k;
	}
}

// the smallest s >= 0 with (m >> s)^2 N (N - 1) < 2^62
int32_t shift_of(int32_t m, int32_t N)
{
	int32_t s = 0;
	const unsigned __int128 pairs = (unsigned __int128)((uint64_t)N * (uint64_t)(N - 1)), lim = (unsigned __int128)1 << 62;
	while ((unsigned __int128)((uint64_t)(m >> s) * (uint64_t)(m >> s)) * pairs >= lim) ++s;
	return s;
}

double t_perma = 0; // seconds of the backend step (or the host loops) of the last command

// one label row lab[A] (1, 0, negative = missing) over q[A][A] with F fraction bits; 0 or a PGA_ERR_* code
int permanova_one(const int32_t *q, int32_t A, const int8_t *lab, int32_t F, int32_t n_perm, uint32_t seed, Perma &r)
{
	std::vector<int32_t> col;
	r = Perma();
	for (int32_t c = 0; c < A; ++c)
		if (lab[c] >= 0) col.push_back(c), r.n1 += lab[c] > 0;
	const int32_t N = r.N = (int32_t)col.size(), n1 = r.n1;
	if (N < 3 || n1 == 0 || n1 == N) return 0;
	if (N > PERMA_MAX_COL) return PGA_ERR_RANGE;
	const size_t n_ = (size_t)N;
	std::vector<int32_t> qc(n_ * n_);
	int32_t m = 0;
	for (size_t i = 0; i < n_; ++i)
		for (size_t j = 0; j < n_; ++j) m = std::max(m, qc[i * n_ + j] = q[(size_t)col[i] * (size_t)A + (size_t)col[j]]);
	if (m == 0) { r.skip = 2; return 0; }
	const int32_t s = shift_of(m, N);
	r.skip = 0, r.Fe = F - s;
	std::vector<uint8_t> y(n_);
	std::vector<uint32_t> label((n_ + 31) / 32, 0);
	for (size_t i = 0; i < n_; ++i)
		if ((y[i] = lab[col[i]] > 0)) label[i >> 5] |= 1u << (i & 31);
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	int rc = 0;
	if (be->pan_permanova != nullptr) {
		const pga_permanova_in_t in{qc.data(), label.data(), N, s, m, n1, n_perm, seed, nullptr, nullptr, nullptr};
		pga_permanova_out_t res{};
		if ((rc = be->pan_permanova(&in, &res)) == 0) r.T = res.t, r.A = res.a, r.B = res.b, r.k = res.k;
	} else permanova_host(qc.data(), y.data(), N, s, n1, n_perm, seed, r);
	t_perma += now_sec() - t0;
	return rc;
}

// q[n][n] as pg_pan_medoids checks it: 0, PGA_ERR_ARG or PGA_ERR_RANGE
int fixed_matrix_ok(const int32_t *q, int32_t n)
{
	const size_t N = (size_t)n;
	bool big = false;
	for (size_t i = 0; i < N; ++i) {
		if (q[i * N + i] != 0) return PGA_ERR_ARG;
		for (size_t j = i + 1; j < N; ++j) {
			if (q[i * N + j] != q[j * N + i] || q[i * N + j] < 0) return PGA_ERR_ARG;
			big |= q[i * N + j] >= MED_IN_MAX;
		}
	}
	return big ? PGA_ERR_RANGE : 0;
}

bool perma_opt_ok(const pg_permanova_opt_t *o)
{
	return o != nullptr && (o->type == PG_DIST_GENE || o->type == PG_DIST_ADJ) && (o->metric == PG_DIST_JACCARD || o->metric == PG_DIST_DIFF) && o->n_perm >= 0 &&
	       o->n_perm <= PERMA_MAX_PERM && o->frac_bits >= 0 && o->frac_bits <= 30;
}

// every row of lab[T][A] over q[A][A]: out[T][7] = N, n1, Fe, T, A, B, k
int permanova_rows(const int32_t *q, int32_t A, const int8_t *lab, int32_t n_trait, int32_t F, const pg_permanova_opt_t *o, int64_t *out)
{
	for (int32_t ti = 0; ti < n_trait; ++ti) {
		Perma r;
		const int rc = permanova_one(q, A, lab + (size_t)ti * (size_t)A, F, o->n_perm, o->seed, r);
		if (rc != 0) return rc;
		int64_t *p = out + 7 * (size_t)ti;
		p[0] = r.N, p[1] = r.n1, p[2] = r.skip ? 0 : r.Fe, p[3] = r.T, p[4] = r.A, p[5] = r.B, p[6] = r.skip ? -1 : r.k;
	}
	return 0;
}

// num / den as ONE long double division (both exact 128-bit integers), times 2^-shift
double ratio(i128 num, i128 den, int32_t shift = 0) { return (double)std::ldexp((long double)num / (long double)den, -shift); }

// ---- Mantel test ------------------------------------------------------------------------------------------------------------------

constexpr int32_t MANTEL_MAX_COL = 16384, MANTEL_MAX_PERM = 2147483646; // the backend's limits (include/pangene_hip.h pga_pan_mantel)

// what one pair of matrices leaves.  skip: 0 = tested, 1 = N < 3, 2 = a constant matrix (va = 0 or vb = 0)
struct Mantel { int32_t N = 0, sx = 0, sy = 0, skip = 1; int64_t Sa = 0, Sb = 0, Saa = 0, Sbb = 0, Z = 0, n_ge = 0, n_le = 0; };

// The backend's step on the host, by the definition: Z of an order as a double loop over i < j, doubled; the identity first, then every
// permutation's order from fisher_yates_order.  a[N][N], b[N][N]
void mantel_host(const int32_t *a, const int32_t *b, int32_t N, int32_t n, uint32_t seed, Mantel &r)
{
	const size_t n_ = (size_t)N;
	std::vector<int32_t> o(n_);
	auto Z = [&]() {
		uint64_t z = 0;
		for (size_t i = 0; i < n_; ++i)
			for (size_t j = i + 1; j < n_; ++j) z += (uint64_t)a[i * n_ + j] * (uint64_t)b[(size_t)o[i] * n_ + (size_t)o[j]];
		return (int64_t)(2 * z); // both orders of the pair
	};
	for (int32_t i = 0; i < N; ++i) o[(size_t)i] = i;
	r.Z = Z();
	r.n_ge = r.n_le = 0;
	for (int32_t p = 1; p <= n; ++p) {
		fisher_yates_order(N, seed, (uint32_t)p, o.data());
		const int64_t zp = Z();
		r.n_ge += zp >= r.Z, r.n_le += zp <= r.Z;
	}
}

double t_mantel = 0; // seconds of the backend step (or the host loops) of the last command

// qx[N][N] against qy[N][N], both checked (symmetric, zero diagonal, entries in [0, 2^29)); 0 or a PGA_ERR_* code
int mantel_core(const int32_t *qx, const int32_t *qy, int32_t N, int32_t n_perm, uint32_t seed, Mantel &r)
{
	r = Mantel();
	r.N = N;
	if (N > MANTEL_MAX_COL) return PGA_ERR_RANGE;
	const size_t n_ = (size_t)N, nn = n_ * n_;
	int32_t mx = 0, my = 0;
	for (size_t k = 0; k < nn; ++k) mx = std::max(mx, qx[k]), my = std::max(my, qy[k]);
	r.sx = shift_of(mx, N), r.sy = shift_of(my, N);
	std::vector<int32_t> a(nn), b(nn);
	for (size_t k = 0; k < nn; ++k) { // (the diagonal is zero)
		const int64_t x = a[k] = qx[k] >> r.sx, y = b[k] = qy[k] >> r.sy;
		r.Sa += x, r.Sb += y, r.Saa += x * x, r.Sbb += y * y;
	}
	if (N < 3) return 0;
	const i128 M = (i128)N * (N - 1);
	if (M * r.Saa - (i128)r.Sa * r.Sa == 0 || M * r.Sbb - (i128)r.Sb * r.Sb == 0) { r.skip = 2; return 0; }
	r.skip = 0;
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	int rc = 0;
	if (be->pan_mantel != nullptr) {
		const pga_mantel_in_t in{a.data(), b.data(), N, mx >> r.sx, my >> r.sy, n_perm, seed, nullptr, nullptr};
		pga_mantel_out_t res{};
		if ((rc = be->pan_mantel(&in, &res)) == 0) r.Z = res.z, r.n_ge = res.n_ge, r.n_le = res.n_le;
	} else mantel_host(a.data(), b.data(), N, n_perm, seed, r);
	t_mantel += now_sec() - t0;
	return rc;
}

bool mantel_opt_ok(const pg_mantel_opt_t *o)
{
	auto type_ok = [](int32_t t) { return t == PG_DIST_GENE || t == PG_DIST_ADJ; };
	auto metric_ok = [](int32_t m) { return m == PG_DIST_JACCARD || m == PG_DIST_DIFF; };
	return o != nullptr && type_ok(o->x_type) && type_ok(o->y_type) && metric_ok(o->x_metric) && metric_ok(o->y_metric) && o->n_perm >= 0 && o->n_perm <= MANTEL_MAX_PERM;
}

// one side of the test: a fixed-point matrix q[names][names] and what the X / Y column prints for it
struct MantelSide { std::string label; std::vector<std::string> names; std::vector<int32_t> q; };

void blank_fields(const std::string &l, std::vector<std::string> &f) // the fields of a line between blanks and tabs
{
	f.clear();
	for (size_t i = 0; i < l.size();) {
		while (i < l.size() && (l[i] == ' ' || l[i] == '\t' || l[i] == '\r')) ++i;
		size_t e = i;
		while (e < l.size() && l[e] != ' ' && l[e] != '\t' && l[e] != '\r') ++e;
		if (e > i) f.emplace_back(l, i, e - i);
		i = e;
	}
}

// An external matrix in either form pangene dist prints: the table ("Asm" and the names, then a name and its values per line) or relaxed
// PHYLIP (a count, then a name and its values per line).  Values by strtod; q = floor(v 2^F + 0.5) with the largest F in [0, 20] that
// keeps every entry below 2^29.  0, or -1 after one line on stderr that names the file and the line
int read_matrix_file(const char *fn, MantelSide &s)
{
	std::vector<std::string> lines, f;
	if (fn == nullptr || read_lines(fn, lines) != 0) { std::fprintf(stderr, "Error: cannot open matrix file %s\n", fn ? fn : "(null)"); return -1; }
	size_t ln = 0;
	for (; ln < lines.size(); ++ln) { blank_fields(lines[ln], f); if (!f.empty()) break; }
	if (ln == lines.size()) { std::fprintf(stderr, "Error: %s: line 1: no header line\n", fn); return -1; }
	const bool table = f[0] == "Asm";
	size_t n = 0;
	s.names.clear();
	if (table) s.names.assign(f.begin() + 1, f.end()), n = s.names.size();
	else {
		const bool digits = f.size() == 1 && f[0].size() <= 9 && f[0].find_first_not_of("0123456789") == std::string::npos;
		if (!digits) { std::fprintf(stderr, "Error: %s: line %zu: neither an Asm header line nor a count\n", fn, ln + 1); return -1; }
		n = (size_t)std::strtoul(f[0].c_str(), nullptr, 10);
	}
	std::vector<double> v;
	std::vector<size_t> row_line;
	double vmax = 0;
	size_t last = ln + 1;
	for (++ln; ln < lines.size(); ++ln) {
		blank_fields(lines[ln], f);
		if (f.empty()) continue;
		const size_t row = row_line.size();
		last = ln + 1;
		if (row == n) { std::fprintf(stderr, "Error: %s: line %zu: the matrix is not square: more than %zu rows\n", fn, ln + 1, n); return -1; }
		if (f.size() != n + 1) { std::fprintf(stderr, "Error: %s: line %zu: the matrix is not square: %zu values in a row, %zu columns\n", fn, ln + 1, f.size() - 1, n); return -1; }
		if (!table) s.names.push_back(f[0]);
		else if (f[0] != s.names[row]) { std::fprintf(stderr, "Error: %s: line %zu: row %s where the header has %s\n", fn, ln + 1, f[0].c_str(), s.names[row].c_str()); return -1; }
		for (size_t j = 0; j < n; ++j) {
			char *end = nullptr;
			const double x = std::strtod(f[j + 1].c_str(), &end);
			if (end == f[j + 1].c_str() || *end != 0 || !std::isfinite(x) || !(x >= 0)) {
				std::fprintf(stderr, "Error: %s: line %zu: value %s is not a finite number >= 0\n", fn, ln + 1, f[j + 1].c_str());
				return -1;
			}
			if (j == row && x != 0) { std::fprintf(stderr, "Error: %s: line %zu: the diagonal value %s is not 0\n", fn, ln + 1, f[j + 1].c_str()); return -1; }
			v.push_back(x), vmax = std::max(vmax, x);
		}
		row_line.push_back(ln + 1);
	}
	if (row_line.size() != n) { std::fprintf(stderr, "Error: %s: line %zu: the matrix is not square: %zu rows, %zu columns\n", fn, last, row_line.size(), n); return -1; }
	std::unordered_map<std::string, size_t> at;
	for (size_t i = 0; i < n; ++i)
		if (!at.emplace(s.names[i], i).second) { std::fprintf(stderr, "Error: %s: line %zu: assembly %s is named twice\n", fn, table ? 1 : row_line[i], s.names[i].c_str()); return -1; }
	int F = 20;
	while (F >= 0 && !(std::floor(std::ldexp(vmax, F) + 0.5) < 536870912.0)) --F;
	if (F < 0) { std::fprintf(stderr, "Error: %s: the largest value %g does not fit 29 bits\n", fn, vmax); return -1; }
	s.q.resize(n * n);
	for (size_t k = 0; k < n * n; ++k) s.q[k] = (int32_t)std::floor(std::ldexp(v[k], F) + 0.5);
	for (size_t i = 0; i < n; ++i)
		for (size_t j = 0; j < i; ++j)
			if (s.q[i * n + j] != s.q[j * n + i]) {
				std::fprintf(stderr, "Error: %s: line %zu: the matrix is not symmetric: %s to %s and back differ\n", fn, row_line[i], s.names[i].c_str(), s.names[j].c_str());
				return -1;
			}
	s.label = "file";
	return 0;
}

// a run's results into the caller's arrays; rec takes the first rec_cap records
void medoids_copy(const Medoids &r, int32_t *medoid, int32_t *label, int32_t *dist, int32_t *size, int64_t *sums, int64_t *rec, int32_t rec_cap, int32_t *n_rec,
                  int32_t *n_swap, int64_t *td, int32_t *converged)
{
	std::copy(r.medoid.begin(), r.medoid.end(), medoid), std::copy(r.label.begin(), r.label.end(), label), std::copy(r.dist.begin(), r.dist.end(), dist);
	std::copy(r.size.begin(), r.size.end(), size), std::copy(r.sums.begin(), r.sums.end(), sums);
	const size_t nr = r.rec.size() / 3;
	std::copy(r.rec.begin(), r.rec.begin() + (std::ptrdiff_t)(3 * std::min(nr, (size_t)std::max(rec_cap, 0))), rec);
	*n_rec = (int32_t)nr, *n_swap = r.n_swap, *td = r.td, *converged = r.converged;
}

} // namespace

int tree_joins(const std::vector<uint32_t> &bits, int32_t M, int32_t A, int32_t metric, int32_t method, int64_t *rec)
{
	if (A < 3) return 0;
	std::vector<int32_t> q;
	int32_t F;
	return tree_records(bits, M, A, metric, method, q, rec, &F);
}

int permanova_run(const char *route, const std::vector<std::string> &trait, const std::vector<int8_t> &lab, const std::vector<uint32_t> &bits, int32_t M, int32_t A,
                  const pg_permanova_opt_t *o, double t_start)
{
	if (!perma_opt_ok(o)) return PGA_ERR_ARG;
	const double t_prep = now_sec() - t_start;
	const size_t nn = (size_t)A * (size_t)A;
	std::vector<int32_t> S(nn), q(nn);
	int32_t F = 20;
	if (A > 0) {
		int rc = shared_count(bits, M, A, S.data());
		if (rc != 0) return rc;
		if ((rc = to_fixed(S.data(), A, o->metric, q.data(), &F)) != 0) return rc;
	}
	t_perma = 0;
	OutBuf ob;
	std::string &s = ob.s;
	s = "Trait\tN\tn1\tn0\tFbits\tSS_total\tSS_within\tF\tR2\tn_ge\tp_perm\n";
	char b[256];
	for (size_t ti = 0; ti < trait.size(); ++ti) {
		Perma r;
		const int rc = permanova_one(q.data(), A, lab.data() + ti * (size_t)A, F, o->n_perm, o->seed, r);
		if (rc != 0) return rc;
		if (r.skip) {
			std::fprintf(stderr, "Note: trait %s has %s over its %d assemblies; skipped\n", trait[ti].c_str(),
			             r.skip == 2 ? "no distance above zero" : r.N < 3 ? "fewer than 3 values" : "one group only", r.N);
			continue;
		}
		const int64_t N = r.N, n1 = r.n1, n0 = N - n1;
		const i128 X = (i128)N * r.A - (i128)(2 * n1) * r.B + (i128)n1 * r.T; // 2 n0 n1 SSW
		const i128 tn = (i128)r.T * (n0 * n1), Y = tn - (i128)N * X;          // 2 N n0 n1 (SST - SSW)
		std::snprintf(b, sizeof(b), "\t%d\t%d\t%d\t%d\t%.6f\t%.6f\t", (int)N, (int)n1, (int)n0, r.Fe, ratio(r.T, 2 * N, 2 * r.Fe), ratio(X, 2 * n0 * n1, 2 * r.Fe));
		s += trait[ti], s += b;
		if (X == 0) s += "inf";
		else std::snprintf(b, sizeof(b), "%.6f", ratio(Y * (N - 2), (i128)N * X)), s += b;
		std::snprintf(b, sizeof(b), "\t%.4f\t", ratio(Y, tn));
		s += b;
		if (o->n_perm > 0) std::snprintf(b, sizeof(b), "%lld\t%.6f\n", (long long)r.k, ((double)r.k + 1.0) / ((double)o->n_perm + 1.0));
		else std::snprintf(b, sizeof(b), "NA\tNA\n");
		s += b;
	}
	ob.finish();
	if (std::getenv("PANGENE_PERMANOVA_TIMING") != nullptr)
		std::fprintf(stderr, "[permanova-timing] route=%s items=%d assemblies=%d traits=%zu perms=%d prep_ms=%.3f stat_ms=%.3f all_ms=%.3f\n", route, M, A, trait.size(),
		             o->n_perm, t_prep * 1e3, t_perma * 1e3, (now_sec() - t_start) * 1e3);
	return 0;
}

namespace {

const char *mantel_spec(int32_t type, int32_t metric)
{
	return type == PG_DIST_GENE ? (metric == PG_DIST_JACCARD ? "gene:jaccard" : "gene:diff") : (metric == PG_DIST_JACCARD ? "adj:jaccard" : "adj:diff");
}

// one side from the items of `type` (items: dist_items_file or dist_items_graph with its first argument bound): 0, 1 when the items
// cannot be had, or a PGA_ERR_* code
template <class Items> int mantel_side(Items &items, int32_t type, int32_t metric, MantelSide &s)
{
	std::vector<uint32_t> bits;
	int32_t M = 0;
	if (items(type, s.names, bits, M) != 0) return 1;
	const int32_t A = (int32_t)s.names.size();
	const size_t nn = (size_t)A * (size_t)A;
	std::vector<int32_t> S(nn);
	s.q.assign(nn, 0);
	int32_t F = 20;
	if (A > 0) {
		int rc = shared_count(bits, M, A, S.data());
		if (rc != 0) return rc;
		if ((rc = to_fixed(S.data(), A, metric, s.q.data(), &F)) != 0) return rc;
	}
	s.label = mantel_spec(type, metric);
	return 0;
}

// the assemblies both sides name, in X's order; a name on one side only gets a note and is left out.  Then the test and the text
int mantel_write(const char *route, const MantelSide &X, const MantelSide &Y, const pg_mantel_opt_t *o, double t_start)
{
	const double t_prep = now_sec() - t_start;
	std::unordered_map<std::string, size_t> at;
	for (size_t k = 0; k < Y.names.size(); ++k) at.emplace(Y.names[k], k);
	std::vector<size_t> ix, iy;
	std::vector<uint8_t> used(Y.names.size(), 0);
	for (size_t i = 0; i < X.names.size(); ++i) {
		const auto it = at.find(X.names[i]);
		if (it == at.end()) { std::fprintf(stderr, "Note: assembly %s is in %s only; left out\n", X.names[i].c_str(), X.label.c_str()); continue; }
		ix.push_back(i), iy.push_back(it->second), used[it->second] = 1;
	}
	for (size_t k = 0; k < Y.names.size(); ++k)
		if (!used[k]) std::fprintf(stderr, "Note: assembly %s is in %s only; left out\n", Y.names[k].c_str(), Y.label.c_str());
	const size_t n_ = ix.size(), nx = X.names.size(), ny = Y.names.size();
	std::vector<int32_t> qx(n_ * n_), qy(n_ * n_);
	for (size_t i = 0; i < n_; ++i)
		for (size_t j = 0; j < n_; ++j) qx[i * n_ + j] = X.q[ix[i] * nx + ix[j]], qy[i * n_ + j] = Y.q[iy[i] * ny + iy[j]];
	t_mantel = 0;
	Mantel r;
	const int rc = mantel_core(qx.data(), qy.data(), (int32_t)n_, o->n_perm, o->seed, r);
	if (rc != 0) return rc;
	OutBuf ob;
	std::string &s = ob.s;
	s = "X\tY\tN\tr\tn_ge\tn_le\tp_greater\tp_less\n";
	if (r.skip) std::fprintf(stderr, "Note: %s over the %d assemblies; not tested\n", r.skip == 2 ? "a matrix has one value only" : "fewer than 3 assemblies", r.N);
	else {
		const i128 M = (i128)r.N * (r.N - 1), num = M * r.Z - (i128)r.Sa * r.Sb, va = M * r.Saa - (i128)r.Sa * r.Sa, vb = M * r.Sbb - (i128)r.Sb * r.Sb;
		const long double rho = ((long double)num / sqrtl((long double)va)) / sqrtl((long double)vb);
		char b[256];
		std::snprintf(b, sizeof(b), "\t%d\t%.4Lf\t%lld\t%lld\t", r.N, rho, (long long)r.n_ge, (long long)r.n_le);
		s += X.label, s += '\t', s += Y.label, s += b;
		if (o->n_perm > 0) std::snprintf(b, sizeof(b), "%.6f\t%.6f\n", ((double)r.n_ge + 1.0) / ((double)o->n_perm + 1.0), ((double)r.n_le + 1.0) / ((double)o->n_perm + 1.0));
		else std::snprintf(b, sizeof(b), "NA\tNA\n");
		s += b;
	}
	ob.finish();
	if (std::getenv("PANGENE_MANTEL_TIMING") != nullptr)
		std::fprintf(stderr, "[mantel-timing] route=%s assemblies=%d perms=%d prep_ms=%.3f stat_ms=%.3f all_ms=%.3f\n", route, r.N, o->n_perm, t_prep * 1e3,
		             t_mantel * 1e3, (now_sec() - t_start) * 1e3);
	return 0;
}

// both sides, then mantel_write: 0, 1 (the items cannot be had), 2 (a bad matrix file, its line is on stderr) or a PGA_ERR_* code
template <class Items> int mantel_run(const char *route, Items items, const char *mat_fn, const pg_mantel_opt_t *o, double t_start)
{
	if (!mantel_opt_ok(o)) return PGA_ERR_ARG;
	MantelSide X, Y;
	int rc = mantel_side(items, o->x_type, o->x_metric, X);
	if (rc != 0) return rc;
	if (mat_fn != nullptr) { if (read_matrix_file(mat_fn, Y) != 0) return 2; }
	else if ((rc = mantel_side(items, o->y_type, o->y_metric, Y)) != 0) return rc;
	return mantel_write(route, X, Y, o, t_start);
}

} // namespace

} // namespace pgx

using namespace pgx;

extern "C" {

void pg_tree_opt_init(pg_tree_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->method = PG_TREE_NJ;
}

int pg_tree_file(const char *gfa_fn, const pg_tree_opt_t *o)
{
	const double t0 = now_sec();
	std::vector<std::string> names;
	std::vector<uint32_t> bits;
	int32_t M;
	if (dist_items_file(gfa_fn, o->type, names, bits, M) != 0) return cannot_open(gfa_fn);
	const int rc = tree_run("file", names, bits, M, o, t0);
	if (rc != 0) { std::fprintf(stderr, "Error: pangene tree: %s\n", backend_default()->strerror(rc)); return -2; }
	return 0;
}

void pg_write_tree(pg_graph_t *q, const pg_tree_opt_t *o)
{
	const double t0 = now_sec();
	std::vector<std::string> names;
	std::vector<uint32_t> bits;
	int32_t M;
	if (dist_items_graph(q, o->type, names, bits, M) != 0) return;
	const int rc = tree_run("memory", names, bits, M, o, t0);
	if (rc != 0) set_error(rc, "pg_write_tree");
}

int pg_pan_join(const int32_t *q, int32_t n, int32_t method, int64_t *rec) { return join_run(q, n, method, rec); }

int pg_pan_tree(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, int32_t method, int64_t *rec, int32_t *frac_bits)
{
	if ((metric != PG_DIST_JACCARD && metric != PG_DIST_DIFF) || (method != PG_TREE_NJ && method != PG_TREE_UPGMA)) return PGA_ERR_ARG;
	if (n_item < 0 || n_asm < 3 || ((size_t)n_item > 0 && presence == nullptr) || rec == nullptr || frac_bits == nullptr) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	std::vector<int32_t> q;
	return tree_records(bits, n_item, n_asm, metric, method, q, rec, frac_bits);
}

static bool boot_args_ok(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, int32_t method)
{
	return (metric == PG_DIST_JACCARD || metric == PG_DIST_DIFF) && (method == PG_TREE_NJ || method == PG_TREE_UPGMA) && n_item >= 0 && n_asm >= 3 &&
	       !((size_t)n_item > 0 && presence == nullptr);
}

int pg_pan_boot(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, int32_t method, int32_t n_boot, uint32_t seed, int64_t *rec,
                int32_t *frac_bits, int32_t *count)
{
	if (!boot_args_ok(presence, n_item, n_asm, metric, method) || n_boot < 0 || rec == nullptr || frac_bits == nullptr || count == nullptr) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	std::vector<int32_t> q;
	const int rc = tree_records(bits, n_item, n_asm, metric, method, q, rec, frac_bits);
	return rc != 0 ? rc : boot_support(bits, n_item, n_asm, metric, method, n_boot, seed, rec, count);
}

int pg_pan_boot_records(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, int32_t method, uint32_t seed, int32_t first, int32_t n,
                        int64_t *rec_out)
{
	if (!boot_args_ok(presence, n_item, n_asm, metric, method) || first < 1 || n < 0 || (int64_t)first + n - 1 > INT32_MAX || (n > 0 && rec_out == nullptr)) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	const size_t stride = 6 * (size_t)(method == PG_TREE_NJ ? n_asm - 2 : n_asm - 1);
	int64_t *at = rec_out;
	return boot_walk(bits, n_item, n_asm, metric, method, seed, first, n, [&](const int64_t *r, int32_t k) {
		std::memcpy(at, r, sizeof(int64_t) * stride * (size_t)k);
		at += stride * (size_t)k;
	});
}

void pg_cluster_opt_init(pg_cluster_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->k_lo = o->k_hi = 2, o->max_iter = 1000;
}

int pg_cluster_file(const char *gfa_fn, const pg_cluster_opt_t *o)
{
	const double t0 = now_sec();
	std::vector<std::string> names;
	std::vector<uint32_t> bits;
	int32_t M;
	if (dist_items_file(gfa_fn, o->type, names, bits, M) != 0) return cannot_open(gfa_fn);
	const int rc = cluster_run("file", names, bits, M, o, t0);
	if (rc != 0) { std::fprintf(stderr, "Error: pangene cluster: %s\n", backend_default()->strerror(rc)); return -2; }
	return 0;
}

void pg_write_cluster(pg_graph_t *q, const pg_cluster_opt_t *o)
{
	const double t0 = now_sec();
	std::vector<std::string> names;
	std::vector<uint32_t> bits;
	int32_t M;
	if (dist_items_graph(q, o->type, names, bits, M) != 0) return;
	const int rc = cluster_run("memory", names, bits, M, o, t0);
	if (rc != 0) set_error(rc, "pg_write_cluster");
}

int pg_pan_medoids(const int32_t *q, int32_t n, int32_t k, int32_t max_iter, int32_t *medoid, int32_t *label, int32_t *dist, int32_t *size, int64_t *sums, int64_t *rec,
                   int32_t rec_cap, int32_t *n_rec, int32_t *n_swap, int64_t *td, int32_t *converged)
{
	if (medoid == nullptr || label == nullptr || dist == nullptr || size == nullptr || sums == nullptr || (rec == nullptr && rec_cap > 0) || n_rec == nullptr ||
	    n_swap == nullptr || td == nullptr || converged == nullptr) return PGA_ERR_ARG;
	Medoids r;
	const int rc = medoids_run(q, n, k, max_iter, r);
	if (rc == 0) medoids_copy(r, medoid, label, dist, size, sums, rec, rec_cap, n_rec, n_swap, td, converged);
	return rc;
}

int pg_pan_cluster(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, int32_t k, int32_t max_iter, int32_t *medoid, int32_t *label, int32_t *dist,
                   int32_t *size, int64_t *sums, int64_t *rec, int32_t rec_cap, int32_t *n_rec, int32_t *n_swap, int64_t *td, int32_t *converged, int32_t *frac_bits)
{
	if ((metric != PG_DIST_JACCARD && metric != PG_DIST_DIFF) || n_item < 0 || n_asm < 3 || ((size_t)n_item > 0 && presence == nullptr) || frac_bits == nullptr) return PGA_ERR_ARG;
	if (medoid == nullptr || label == nullptr || dist == nullptr || size == nullptr || sums == nullptr || (rec == nullptr && rec_cap > 0) || n_rec == nullptr ||
	    n_swap == nullptr || td == nullptr || converged == nullptr) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	const size_t nn = (size_t)n_asm * (size_t)n_asm;
	std::vector<int32_t> S(nn), q(nn);
	int rc = shared_count(bits, n_item, n_asm, S.data());
	if (rc != 0) return rc;
	if ((rc = to_fixed(S.data(), n_asm, metric, q.data(), frac_bits)) != 0) return rc;
	Medoids r;
	if ((rc = medoids_run(q.data(), n_asm, k, max_iter, r)) == 0) medoids_copy(r, medoid, label, dist, size, sums, rec, rec_cap, n_rec, n_swap, td, converged);
	return rc;
}

void pg_permanova_opt_init(pg_permanova_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->n_perm = 1000, o->seed = 11, o->frac_bits = 20;
}

int pg_pan_permanova(const int32_t *q, int32_t n, const int8_t *labels, int32_t n_trait, const pg_permanova_opt_t *o, int64_t *out)
{
	if (n < 0 || n_trait < 0 || !perma_opt_ok(o) || (n > 0 && q == nullptr)) return PGA_ERR_ARG;
	if (((size_t)n_trait * (size_t)n > 0 && labels == nullptr) || (n_trait > 0 && out == nullptr)) return PGA_ERR_ARG;
	const int rc = fixed_matrix_ok(q, n);
	return rc != 0 ? rc : permanova_rows(q, n, labels, n_trait, o->frac_bits, o, out);
}

int pg_pan_permanova_presence(const uint8_t *presence, int32_t n_item, int32_t n_asm, const int8_t *labels, int32_t n_trait, const pg_permanova_opt_t *o,
                              int64_t *out, int32_t *frac_bits)
{
	if (n_item < 0 || n_asm < 0 || n_trait < 0 || !perma_opt_ok(o) || frac_bits == nullptr || ((size_t)n_item * (size_t)n_asm > 0 && presence == nullptr)) return PGA_ERR_ARG;
	if (((size_t)n_trait * (size_t)n_asm > 0 && labels == nullptr) || (n_trait > 0 && out == nullptr)) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	const size_t nn = (size_t)n_asm * (size_t)n_asm;
	std::vector<int32_t> S(nn), q(nn);
	*frac_bits = 20;
	if (n_asm > 0) {
		int rc = shared_count(bits, n_item, n_asm, S.data());
		if (rc != 0) return rc;
		if ((rc = to_fixed(S.data(), n_asm, o->metric, q.data(), frac_bits)) != 0) return rc;
	}
	return permanova_rows(q.data(), n_asm, labels, n_trait, *frac_bits, o, out);
}

void pg_mantel_opt_init(pg_mantel_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->x_type = PG_DIST_GENE, o->x_metric = PG_DIST_JACCARD, o->y_type = PG_DIST_ADJ, o->y_metric = PG_DIST_JACCARD, o->n_perm = 1000, o->seed = 11;
}

int pg_mantel_file(const char *gfa_fn, const char *mat_fn, const pg_mantel_opt_t *o)
{
	const double t0 = now_sec();
	if (o == nullptr) { std::fprintf(stderr, "Error: pan_mantel: no options\n"); return -2; }
	auto items = [&](int32_t type, std::vector<std::string> &names, std::vector<uint32_t> &bits, int32_t &M) { return dist_items_file(gfa_fn, type, names, bits, M); };
	const int rc = mantel_run("file", items, mat_fn, o, t0);
	if (rc == 1) return cannot_open(gfa_fn);
	if (rc == 2) return -3;
	if (rc != 0) { std::fprintf(stderr, "Error: pan_mantel: %s\n", backend_default()->strerror(rc)); return -2; }
	return 0;
}

void pg_write_mantel(pg_graph_t *q, const char *mat_fn, const pg_mantel_opt_t *o)
{
	const double t0 = now_sec();
	if (o == nullptr) { set_error(PGA_ERR_ARG, "pg_write_mantel"); return; }
	auto items = [&](int32_t type, std::vector<std::string> &names, std::vector<uint32_t> &bits, int32_t &M) { return dist_items_graph(q, type, names, bits, M); };
	const int rc = mantel_run("memory", items, mat_fn, o, t0);
	if (rc == 1) return;
	if (rc == 2) set_error(PGA_ERR_ARG, "pg_write_mantel: bad matrix file");
	else if (rc != 0) set_error(rc, "pg_write_mantel");
}

int pg_pan_mantel(const int32_t *qx, const int32_t *qy, int32_t n, const pg_mantel_opt_t *o, int64_t *out)
{
	if (n < 0 || !mantel_opt_ok(o) || out == nullptr || (n > 0 && (qx == nullptr || qy == nullptr))) return PGA_ERR_ARG;
	if (n > MANTEL_MAX_COL) return PGA_ERR_RANGE; // (before the matrices are looked at)
	int rc = fixed_matrix_ok(qx, n);
	if (rc == 0) rc = fixed_matrix_ok(qy, n);
	if (rc != 0) return rc;
	Mantel r;
	if ((rc = mantel_core(qx, qy, n, o->n_perm, o->seed, r)) != 0) return rc;
	out[0] = r.N, out[1] = r.sx, out[2] = r.sy, out[3] = r.Sa, out[4] = r.Sb, out[5] = r.Saa, out[6] = r.Sbb;
	out[7] = r.skip ? 0 : r.Z, out[8] = r.skip ? -1 : r.n_ge, out[9] = r.skip ? -1 : r.n_le;
	return 0;
}

} // extern "C"
