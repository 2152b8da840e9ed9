// pan_tree.hpp -- a tree of the assemblies from their pairwise distances (pg_tree_file, pg_write_tree, pg_pan_join, pg_pan_tree;
// include/pangene_amd.h).  The distances of pangene dist become fixed-point integers, neighbour-joining or UPGMA joins them in integer
// arithmetic (DESIGN.md section 8 "Trees": every sum is an integer sum, ties go to the smallest slot numbers), and only the Newick text
// is floating point.  The joins run on the backend (pga_pan_join), or as the plain loops below when the backend has no such entry.
// Bootstrap support (pg_pan_boot, pg_pan_boot_records, pangene tree -b; DESIGN.md section 8 "Bootstrap"): the replicates' records come from
// the backend in chunks (pga_pan_boot), or from the plain loops below, and are folded into per-join counts here, in code both builds share.
// First the two things the four commands of tree.cpp share: the fixed-point distances (fixed_dist) and where a command's items come
// from (ItemSource, file_result, graph_result).

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

// bit rows bits[A][(M + 31) / 32] -> q[A][A] = their distances * 2^F.  A == 0: nothing, and *frac_bits stays what it was
int fixed_dist(const std::vector<uint32_t> &bits, int32_t M, int32_t A, int32_t metric, std::vector<int32_t> &q, int32_t *frac_bits)
{
	const size_t nn = (size_t)A * (size_t)A;
	q.assign(nn, 0);
	if (A == 0) return 0;
	std::vector<int32_t> S(nn);
	const int rc = shared_count(bits, M, A, S.data());
	return rc != 0 ? rc : to_fixed(S.data(), A, metric, q.data(), frac_bits);
}

// Where a command's items come from: a GFA file, or the graph in memory.  A run takes the source, reads the items of the type(s) its
// options name and returns 0, a PGA_ERR_* code, PAN_NO_ITEMS (the items cannot be had) or PAN_BAD_FILE (its second file -- traits, a
// matrix -- was turned down, the line is on stderr); file_result and graph_result make of that what a pg_*_file entry returns and
// what a pg_write_* entry records.
struct ItemSource {
	const char *gfa_fn;
	pg_graph_t *g;
	bool memory;
	const char *route() const { return memory ? "memory" : "file"; }
	int operator()(int32_t type, std::vector<std::string> &names, std::vector<uint32_t> &bits, int32_t &M, std::vector<std::string> *item_names = nullptr) const
	{
		return memory ? dist_items_graph(g, type, names, bits, M, item_names) : dist_items_file(gfa_fn, type, names, bits, M, item_names);
	}
};
inline ItemSource items_of_file(const char *gfa_fn) { return ItemSource{gfa_fn, nullptr, false}; }
inline ItemSource items_of_graph(pg_graph_t *g) { return ItemSource{nullptr, g, true}; }
enum { PAN_NO_ITEMS = 1 << 20, PAN_BAD_FILE };

int file_result(int rc, const char *gfa_fn, const char *cmd)
{
	if (rc == PAN_NO_ITEMS) return cannot_open(gfa_fn);
	if (rc == PAN_BAD_FILE) return -3;
	if (rc != 0) { std::fprintf(stderr, "Error: %s: %s\n", cmd, backend_default()->strerror(rc)); return -2; }
	return 0;
}

void graph_result(int rc, const char *where, const char *bad_file = nullptr)
{
	if (rc == PAN_BAD_FILE) set_error(PGA_ERR_ARG, bad_file);
	else if (rc != 0 && rc != PAN_NO_ITEMS) set_error(rc, where);
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

// Replicate b of the definition as plain loops: the draws, the resampled rows, fixed_dist, join_host.  bits[A][W]
int boot_host(const std::vector<uint32_t> &bits, int32_t M, int32_t A, int32_t metric, int32_t method, uint32_t seed, uint32_t b, int64_t *rec)
{
	const size_t W = ((size_t)M + 31) / 32;
	std::vector<uint32_t> rows((size_t)A * W, 0);
	const uint64_t x0 = mix64((uint64_t)seed << 32 | (uint64_t)b);
	for (int32_t t = 0; t < M; ++t) {
		const uint64_t m = mix64(x0 + (uint64_t)(t + 1) * 0x9E3779B97F4A7C15ull) % (uint64_t)M;
		for (size_t a = 0; a < (size_t)A; ++a)
			if (bits[a * W + (size_t)(m >> 5)] >> (m & 31) & 1u) rows[a * W + (size_t)(t >> 5)] |= 1u << (t & 31);
	}
	std::vector<int32_t> q;
	int32_t F;
	const int rc = fixed_dist(rows, M, A, metric, q, &F);
	return rc != 0 ? rc : join_host(q, A, method, rec);
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
	const int rc = fixed_dist(bits, M, A, metric, q, F);
	if (rc != 0) return rc;
	return A >= 3 ? join_run(q.data(), A, method, rec) : 0;
}

int tree_run(const ItemSource &src, const pg_tree_opt_t *o)
{
	const double t_start = now_sec();
	std::vector<std::string> names;
	std::vector<uint32_t> bits;
	int32_t M;
	if (src(o->type, names, bits, M) != 0) return PAN_NO_ITEMS;
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
	report_time(src.route(), M, A, t_prep, now_sec() - t1);
	return 0;
}

} // namespace

int tree_joins(const std::vector<uint32_t> &bits, int32_t M, int32_t A, int32_t metric, int32_t method, int64_t *rec)
{
	if (A < 3) return 0;
	std::vector<int32_t> q;
	int32_t F;
	return tree_records(bits, M, A, metric, method, q, rec, &F);
}

} // namespace pgx

extern "C" {

void pg_tree_opt_init(pg_tree_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->method = PG_TREE_NJ;
}

int pg_tree_file(const char *gfa_fn, const pg_tree_opt_t *o) { return file_result(tree_run(items_of_file(gfa_fn), o), gfa_fn, "pangene tree"); }
void pg_write_tree(pg_graph_t *q, const pg_tree_opt_t *o) { graph_result(tree_run(items_of_graph(q), o), "pg_write_tree"); }

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

} // extern "C"
