// trait.cpp -- gene-trait association (pg_trait_file, pg_write_trait, pg_pan_trait; include/pangene_amd.h): which genes go with a
// binary phenotype of the assemblies.  Per trait the columns that have a value are compacted and every gene becomes a bit row over
// them; the observed counts and the label-permutation counts k_g come from the backend (pga_pan_trait: the permuted label rows are
// made and counted on the device and one integer per gene comes back), or from the plain loops below when the backend has no such
// entry.  Everything the permutation test decides is an integer; phi, the Fisher p and the Benjamini-Hochberg q are computed here,
// for printing only, by code both builds share.
// Lineage-aware pairwise comparisons (pg_pan_pairs, pangene trait -L; DESIGN.md section 8 "Lineage-aware trait test"): the tree of all
// assemblies comes from tree.cpp; per gene and trait the largest set of contrasting leaf pairs on vertex-disjoint paths and its most
// supporting and most opposing pairs come from the backend (pga_pan_pairs: the tree compiled into a postfix program, one lane per gene), or
// from the plain loops over the records below; the two binomial p values are computed here, by code both builds share.
// Quantitative traits (pg_qtrait_file, pg_write_qtrait, pg_pan_qtrait; DESIGN.md section 8 "Quantitative traits"): the same file shape with
// numbers for values; per trait the centred doubled midranks c2 of the columns with a value, per gene a and D = the sum of c2 over its
// columns, and the permutation counts k_g from the backend (pga_pan_qtrait: the permuted value rows as two signed-byte planes, D_p of
// every gene and permutation as an int8 matrix product) or from the plain loops below; U, auc, z, p_wilcox and q_bh are computed here,
// by code both builds share.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>
#include "pg_internal.hpp"
#include "pan_treeprog.hpp"

namespace pgx {
namespace {

constexpr int32_t TRAIT_MAX_COL = 16777215, TRAIT_MAX_GENE = 16777215, TRAIT_MAX_PERM = 2147483646;
constexpr int32_t PAIRS_MAX_LEAF = 65535, PAIRS_DEPTH = 16; // the backend's limits (include/pangene_hip.h pga_pan_pairs)

// order p >= 1 of N columns: make_orders' sequence (curves.cpp)
void make_order(int32_t N, uint32_t seed, uint32_t p, std::vector<int32_t> &o)
{
	o.resize((size_t)N);
	fisher_yates_order(N, seed, p, o.data());
}

// The backend's step on the host, by the definition: every permutation's label row from its order, every eligible gene's count,
// |D_p| >= |D| in 64-bit integers.  bits[G][W], label[W]
void trait_host(const uint32_t *bits, const uint32_t *label, int32_t G, int32_t N, int32_t W, int32_t min_count, int32_t n, uint32_t seed,
                std::vector<int32_t> &a, std::vector<int32_t> &s, std::vector<int32_t> &k)
{
	a.assign((size_t)G, 0), s.assign((size_t)G, 0), k.assign((size_t)G, 0);
	int64_t t = 0;
	for (int32_t w = 0; w < W; ++w) t += __builtin_popcount(label[w]);
	std::vector<int32_t> el;
	std::vector<int64_t> d_abs;
	for (int32_t g = 0; g < G; ++g) {
		const uint32_t *b = bits + (size_t)g * W;
		int32_t ca = 0, cs = 0;
		for (int32_t w = 0; w < W; ++w) ca += __builtin_popcount(b[w]), cs += __builtin_popcount(b[w] & label[w]);
		a[(size_t)g] = ca, s[(size_t)g] = cs;
		if (std::min(ca, N - ca) >= min_count) el.push_back(g), d_abs.push_back(std::llabs((int64_t)cs * N - (int64_t)ca * t));
	}
	std::vector<int32_t> o;
	std::vector<uint32_t> yp((size_t)W);
	for (int32_t p = 1; p <= n && !el.empty(); ++p) {
		make_order(N, seed, (uint32_t)p, o);
		std::fill(yp.begin(), yp.end(), 0u);
		for (int32_t r = 0; r < N; ++r) {
			const int32_t c = o[(size_t)r];
			yp[(size_t)(r >> 5)] |= ((label[c >> 5] >> (c & 31)) & 1u) << (r & 31);
		}
		for (size_t e = 0; e < el.size(); ++e) {
			const uint32_t *b = bits + (size_t)el[e] * W;
			int64_t sp = 0;
			for (int32_t w = 0; w < W; ++w) sp += __builtin_popcount(b[w] & yp[(size_t)w]);
			if (std::llabs(sp * N - (int64_t)a[(size_t)el[e]] * t) >= d_abs[e]) ++k[(size_t)el[e]];
		}
	}
}

double t_count = 0; // seconds of the last counting step (backend or host loops)

bool opt_ok(const pg_trait_opt_t *o)
{
	return o != nullptr && o->n_perm >= 0 && o->n_perm <= TRAIT_MAX_PERM && o->min_count >= 1 && o->max_p == o->max_p && o->lineage >= 0 && o->lineage <= 2;
}

// a, s, k of every gene over the N compacted columns; 0 or a PGA_ERR_* code
int trait_count(const std::vector<uint32_t> &bits, const std::vector<uint32_t> &label, int32_t G, int32_t N, const pg_trait_opt_t *o,
                std::vector<int32_t> &a, std::vector<int32_t> &s, std::vector<int32_t> &k)
{
	if (G > TRAIT_MAX_GENE || N > TRAIT_MAX_COL) return PGA_ERR_RANGE;
	const int32_t W = (N + 31) / 32;
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	int rc = 0;
	if (be->pan_trait != nullptr) {
		const pga_trait_in_t in{bits.data(), label.data(), G, N, o->min_count, o->n_perm, o->seed, nullptr};
		pga_trait_out_t res{};
		rc = be->pan_trait(&in, &res);
		if (rc == 0) a.assign(res.a, res.a + (size_t)G), s.assign(res.s, res.s + (size_t)G), k.assign(res.k, res.k + (size_t)G);
	} else trait_host(bits.data(), label.data(), G, N, W, o->min_count, o->n_perm, o->seed, a, s, k);
	t_count += now_sec() - t0;
	return rc;
}

// One trait over a presence matrix pres[G][A] (nonzero = present) and labels lab[A] (1, 0, -1 = missing)
struct One { int32_t N = 0, t = 0; std::vector<int32_t> a, s, k; std::vector<uint8_t> elig; };

int trait_one(const uint8_t *pres, const int8_t *lab, int32_t G, int32_t A, const pg_trait_opt_t *o, One &r)
{
	std::vector<int32_t> col;
	for (int32_t c = 0; c < A; ++c) if (lab[c] >= 0) col.push_back(c);
	const int32_t N = (int32_t)col.size(), W = (N + 31) / 32;
	r.N = N, r.t = 0;
	std::vector<uint32_t> label((size_t)W, 0);
	for (int32_t i = 0; i < N; ++i) if (lab[col[(size_t)i]] > 0) label[(size_t)(i >> 5)] |= 1u << (i & 31), ++r.t;
	r.a.assign((size_t)G, 0), r.s.assign((size_t)G, 0), r.k.assign((size_t)G, 0), r.elig.assign((size_t)G, 0);
	if (r.t == 0 || r.t == N) return 0; // a constant trait (N = 0 too): nothing to test
	std::vector<uint32_t> bits((size_t)G * W, 0);
	for (int32_t g = 0; g < G; ++g) {
		const uint8_t *row = pres + (size_t)g * A;
		uint32_t *b = bits.data() + (size_t)g * W;
		for (int32_t i = 0; i < N; ++i) if (row[col[(size_t)i]]) b[i >> 5] |= 1u << (i & 31);
	}
	const int rc = trait_count(bits, label, G, N, o, r.a, r.s, r.k);
	if (rc != 0) return rc;
	for (int32_t g = 0; g < G; ++g) r.elig[(size_t)g] = std::min(r.a[(size_t)g], N - r.a[(size_t)g]) >= o->min_count;
	return 0;
}

// two-sided Fisher exact p of the table (N, t, a, s): lf[i] = log i!.  The hypergeometric distribution is unimodal, so the
// probabilities P(x) <= P(s) (1 + 1e-7) are the two tails: walked inwards from both ends
double fisher(const std::vector<double> &lf, int32_t N, int32_t t, int32_t a, int32_t s)
{
	const int32_t lo = std::max(0, a + t - N), hi = std::min(a, t);
	const double base = lf[(size_t)a] + lf[(size_t)(N - a)] + lf[(size_t)t] + lf[(size_t)(N - t)] - lf[(size_t)N];
	auto lp = [&](int32_t x) { return base - lf[(size_t)x] - lf[(size_t)(a - x)] - lf[(size_t)(t - x)] - lf[(size_t)(N - a - t + x)]; };
	const double thr = lp(s) + std::log1p(1e-7);
	double sum = 0;
	int32_t x = lo;
	for (; x <= hi && lp(x) <= thr; ++x) sum += std::exp(lp(x));
	for (int32_t z = hi; z >= x && lp(z) <= thr; --z) sum += std::exp(lp(z));
	return sum < 1.0 ? sum : 1.0;
}


// ---- lineage-aware pairwise comparisons ----

// (pairs_tree and pairs_program, the records as a tree and the tree as the backend's postfix program: pan_treeprog.hpp)

// The backend's step on the host, by the definition and over the records themselves (no program, no packing): per trait row, gene and
// run every node's N and F_s bottom-up in join order.  A value is pairs << 32 | pairs of the run's side in 64 bits, infeasible is
// PH_NONE or below (the sum of two is still far from wrapping).  out[R][G][3]
constexpr int64_t PH_NONE = -((int64_t)1 << 60), PH_PAIR = (int64_t)1 << 32;
struct PairsNode { int64_t N, F[4]; };

void pairs_host(const uint8_t *pres, const int8_t *lab, int32_t G, int32_t A, int32_t R, const std::vector<int32_t> &kid, int32_t *out)
{
	const size_t n_join = kid.size() / 2;
	std::vector<PairsNode> nd((size_t)A + n_join);
	for (int32_t r = 0; r < R; ++r)
		for (int32_t g = 0; g < G; ++g) {
			int32_t *o = out + ((size_t)r * (size_t)G + (size_t)g) * 3;
			o[0] = o[1] = o[2] = 0;
			if (A == 0) continue;
			for (int32_t run = 0; run < 2; ++run) {
				for (int32_t x = 0; x < A; ++x) {
					PairsNode &n = nd[(size_t)x];
					n.N = 0, n.F[0] = n.F[1] = n.F[2] = n.F[3] = PH_NONE;
					const int8_t y = lab[(size_t)r * (size_t)A + (size_t)x];
					if (y >= 0) n.F[(pres[(size_t)g * (size_t)A + (size_t)x] ? 2 : 0) + (y > 0 ? 1 : 0)] = 0;
				}
				for (size_t t = 0; t < n_join; ++t) {
					const PairsNode &a = nd[(size_t)kid[2 * t]], &b = nd[(size_t)kid[2 * t + 1]];
					PairsNode &v = nd[(size_t)A + t];
					v.N = a.N + b.N;
					for (int32_t s = 0; s < 4; ++s) { // the contrasting type of s is 3 - s; 3-0 supports, 2-1 opposes
						const bool supports = s == 0 || s == 3;
						v.N = std::max(v.N, a.F[s] + b.F[3 - s] + PH_PAIR + (supports == (run == 0) ? 1 : 0));
						v.F[s] = std::max(std::max(a.F[s] + b.N, a.N + b.F[s]), PH_NONE);
					}
				}
				const int64_t top = nd.back().N;
				if (run == 0) o[0] = (int32_t)(top >> 32), o[1] = (int32_t)(top & 0xffffffff);
				else o[2] = (int32_t)(top & 0xffffffff);
			}
		}
}

double t_pairs = 0; // seconds of the last pairs step (backend or host loops)

// pairs, supp, opp of every gene and label row over the tree of the records: out[R][G][3].  0 or a PGA_ERR_* code
int pairs_count(const uint8_t *pres, const int8_t *lab, int32_t G, int32_t A, int32_t R, const int64_t *rec, int32_t method, std::vector<int32_t> &out)
{
	if (A > PAIRS_MAX_LEAF || G > TRAIT_MAX_GENE) return PGA_ERR_RANGE;
	std::vector<int32_t> kid;
	if (!pairs_tree(rec, A, method, kid)) return PGA_ERR_ARG;
	const double t0 = now_sec();
	out.assign((size_t)R * (size_t)G * 3, 0);
	const pga_backend_t *be = backend_default();
	int rc = 0;
	if (be->pan_pairs != nullptr) {
		std::vector<uint8_t> op;
		std::vector<int32_t> order;
		if (pairs_program(kid, A, op, order) > PAIRS_DEPTH) return PGA_ERR_RANGE; // (out of reach below 65 536 leaves)
		std::vector<int32_t> pos((size_t)A);
		for (int32_t k = 0; k < A; ++k) pos[(size_t)order[(size_t)k]] = k;
		const size_t W = ((size_t)G + 31) / 32;
		std::vector<uint32_t> bits((size_t)A * W, 0);
		for (int32_t g = 0; g < G; ++g) {
			const uint8_t *row = pres + (size_t)g * (size_t)A;
			for (int32_t x = 0; x < A; ++x)
				if (row[x]) bits[(size_t)pos[(size_t)x] * W + (size_t)(g >> 5)] |= 1u << (g & 31);
		}
		std::vector<int8_t> label((size_t)R * (size_t)A);
		for (int32_t r = 0; r < R; ++r)
			for (int32_t k = 0; k < A; ++k) label[(size_t)r * (size_t)A + (size_t)k] = lab[(size_t)r * (size_t)A + (size_t)order[(size_t)k]];
		const pga_pairs_in_t in{op.data(), bits.data(), label.data(), G, A, R};
		pga_pairs_out_t res{};
		rc = be->pan_pairs(&in, &res);
		if (rc == 0 && !out.empty()) std::memcpy(out.data(), res.out, sizeof(int32_t) * out.size());
	} else pairs_host(pres, lab, G, A, R, kid, out.data());
	t_pairs += now_sec() - t0;
	return rc;
}

// The exact two-sided binomial p at 1/2: min(1, 2 P(X >= max(k, n - k))), 1 for n = 0.  Up to n = 60 the tail is summed in integers and
// the result is the correctly rounded quotient (a sum of 2^-7 prints the same digits everywhere); beyond, from the log-factorial table
// lf (at least n + 1 entries), the small terms first.
double binom_two_sided(const std::vector<double> &lf, int32_t k, int32_t n)
{
	if (n <= 0) return 1.0;
	const int32_t m = std::max(k, n - k);
	double p;
	if (n <= 60) {
		uint64_t c = 1, sum = 0; // c = C(n, x) from x = n down
		for (int32_t x = n; x >= m; --x) {
			sum += c;
			c = c * (uint64_t)x / (uint64_t)(n - x + 1);
		}
		p = std::ldexp((double)sum, 1 - n);
	} else {
		const double base = lf[(size_t)n] - (double)n * std::log(2.0);
		double sum = 0;
		for (int32_t x = n; x >= m; --x) sum += std::exp(base - lf[(size_t)x] - lf[(size_t)(n - x)]);
		p = 2.0 * sum;
	}
	return p < 1.0 ? p : 1.0;
}

std::vector<std::string> split_tab(const std::string &s)
{
	std::vector<std::string> f;
	size_t b = 0;
	for (;;) {
		const size_t e = s.find('\t', b);
		f.push_back(s.substr(b, e == std::string::npos ? e : e - b));
		if (e == std::string::npos) break;
		b = e + 1;
	}
	return f;
}

// The walk over a trait file both commands share: start(T) once the header is read, then field(trait, assembly, text) for every value,
// false for one that is not `what`.  0, or -1 with a message (the line number in it) on stderr
template <class Start, class Field>
int read_trait_file(const char *fn, const std::vector<std::string> &asm_name, std::vector<std::string> &name, const char *what, Start start, Field field)
{
	std::vector<std::string> lines;
	if (fn == nullptr || read_lines(fn, lines) != 0) { std::fprintf(stderr, "Error: cannot open trait file %s\n", fn ? fn : "(null)"); return -1; }
	if (lines.empty()) { std::fprintf(stderr, "Error: %s: line 1: no header line\n", fn); return -1; }
	const std::vector<std::string> h = split_tab(lines[0]);
	const size_t T = h.size() - 1, A = asm_name.size();
	name.assign(h.begin() + 1, h.end());
	start(T);
	std::unordered_map<std::string, int32_t> at;
	for (size_t i = 0; i < A; ++i) at.emplace(asm_name[i], (int32_t)i);
	std::vector<uint8_t> seen(A, 0);
	for (size_t ln = 1; ln < lines.size(); ++ln) {
		const std::string &l = lines[ln];
		if (l.empty() || l[0] == '#') continue;
		const std::vector<std::string> f = split_tab(l);
		if (f.size() != T + 1) { std::fprintf(stderr, "Error: %s: line %zu: %zu fields, the header has %zu\n", fn, ln + 1, f.size(), T + 1); return -1; }
		const auto it = at.find(f[0]);
		if (it == at.end()) { std::fprintf(stderr, "Error: %s: line %zu: no assembly named %s\n", fn, ln + 1, f[0].c_str()); return -1; }
		if (seen[(size_t)it->second]) { std::fprintf(stderr, "Error: %s: line %zu: assembly %s is named twice\n", fn, ln + 1, f[0].c_str()); return -1; }
		seen[(size_t)it->second] = 1;
		for (size_t j = 0; j < T; ++j)
			if (!field(j, (size_t)it->second, f[j + 1])) { std::fprintf(stderr, "Error: %s: line %zu: value %s is not %s\n", fn, ln + 1, f[j + 1].c_str(), what); return -1; }
	}
	return 0;
}

} // namespace

int read_traits(const char *fn, const std::vector<std::string> &asm_name, Traits &tr)
{
	const size_t A = asm_name.size();
	return read_trait_file(fn, asm_name, tr.name, "1, 0 or NA", [&](size_t T) { tr.lab.assign(T * A, (int8_t)-1); },
	                       [&](size_t j, size_t c, const std::string &v) {
		                       int8_t x;
		                       if (v == "1") x = 1; else if (v == "0") x = 0; else if (v == "NA" || v.empty()) x = -1; else return false;
		                       tr.lab[j * A + c] = x;
		                       return true;
	                       });
}

namespace {

// NA or empty: missing (NaN); otherwise a number strtod consumes entirely, with a finite result
bool qtrait_value(const std::string &v, double &x)
{
	x = std::nan("");
	if (v.empty() || v == "NA") return true;
	char *e;
	const double y = std::strtod(v.c_str(), &e);
	if (e != v.c_str() + v.size() || !std::isfinite(y)) return false;
	x = y;
	return true;
}

} // namespace

int read_qtraits(const char *fn, const std::vector<std::string> &asm_name, QTraits &tr)
{
	const size_t A = asm_name.size();
	return read_trait_file(fn, asm_name, tr.name, "a finite number or NA", [&](size_t T) { tr.val.assign(T * A, std::nan("")); },
	                       [&](size_t j, size_t c, const std::string &v) { return qtrait_value(v, tr.val[j * A + c]); });
}

namespace {

// PANGENE_TRAIT_TIMING=1: one line on stderr per call
void report_time(const char *route, int32_t G, int32_t A, size_t T, int32_t n, double t_all)
{
	if (std::getenv("PANGENE_TRAIT_TIMING") == nullptr) return;
	std::fprintf(stderr, "[trait-timing] route=%s genes=%d assemblies=%d traits=%zu perms=%d count_ms=%.3f all_ms=%.3f\n", route, G, A, T, n, t_count * 1e3, t_all * 1e3);
}

// the same for -L: a second line, so that the first stays what it was
void report_lineage_time(int32_t rows, double t_tree)
{
	if (std::getenv("PANGENE_TRAIT_TIMING") == nullptr) return;
	std::fprintf(stderr, "[trait-lineage-timing] rows=%d tree_ms=%.3f pairs_ms=%.3f\n", rows, t_tree * 1e3, t_pairs * 1e3);
}

// every trait of tr over pres[G][A]: counts, statistics, lines.  0 or a PGA_ERR_* code; nothing is written unless every trait went through
int trait_run(const char *route, const std::vector<std::string> &gene, const std::vector<uint8_t> &pres, int32_t A, const Traits &tr, const pg_trait_opt_t *o,
              double t_start)
{
	if (!opt_ok(o)) return PGA_ERR_ARG;
	if (A > TRAIT_MAX_COL) return PGA_ERR_RANGE;
	const int32_t G = (int32_t)gene.size();
	t_count = t_pairs = 0;
	OutBuf ob;
	std::string &out = ob.s;
	out = "Trait\tGene\tN\tnT\tnG\tnTG\tphi\tp_fisher\tq_bh\tn_ge\tp_perm";
	out += o->lineage ? "\tpairs\tsupp\topp\tp_pair_best\tp_pair_worst\n" : "\n";
	char b[160];
	// -L: the tree of ALL assemblies over the genes (pangene tree -t gene -m jaccard), and the pair counts of every trait that has two
	// values, in one backend call; pc[row_of[ti]][g][3]
	std::vector<int32_t> pc, row_of(tr.name.size(), -1);
	double t_tree = 0;
	if (o->lineage) {
		if (A > PAIRS_MAX_LEAF) return PGA_ERR_RANGE;
		std::vector<int8_t> rows;
		for (size_t ti = 0; ti < tr.name.size(); ++ti) {
			const int8_t *lab = tr.lab.data() + ti * (size_t)A;
			int32_t n0 = 0, n1 = 0;
			for (int32_t c = 0; c < A; ++c) n0 += lab[c] == 0, n1 += lab[c] > 0;
			if (n0 == 0 || n1 == 0) continue;
			row_of[ti] = (int32_t)(rows.size() / (size_t)std::max(A, 1));
			rows.insert(rows.end(), lab, lab + A);
		}
		const int32_t method = o->lineage == 1 ? PG_TREE_NJ : PG_TREE_UPGMA;
		std::vector<int64_t> rec((size_t)6 * (size_t)std::max(A, 1));
		const double t0 = now_sec();
		std::vector<uint32_t> bits;
		pack_cols(pres.data(), G, A, bits);
		int rc = tree_joins(bits, G, A, PG_DIST_JACCARD, method, rec.data());
		t_tree = now_sec() - t0;
		if (rc == 0) rc = pairs_count(pres.data(), rows.data(), G, A, (int32_t)(rows.size() / (size_t)std::max(A, 1)), rec.data(), method, pc);
		if (rc != 0) return rc;
	}
	for (size_t ti = 0; ti < tr.name.size(); ++ti) {
		One r;
		const int rc = trait_one(pres.data(), tr.lab.data() + ti * (size_t)A, G, A, o, r);
		if (rc != 0) return rc;
		const int32_t N = r.N, t = r.t;
		if (t == 0 || t == N) { std::fprintf(stderr, "Note: trait %s has one value over its %d assemblies; skipped\n", tr.name[ti].c_str(), N); continue; }
		std::vector<double> lf((size_t)N + 1);
		for (int32_t i = 0; i <= N; ++i) lf[(size_t)i] = std::lgamma((double)i + 1.0);
		std::vector<int32_t> el;
		for (int32_t g = 0; g < G; ++g) if (r.elig[(size_t)g]) el.push_back(g);
		const size_t m = el.size();
		std::vector<double> pf(m), q;
		for (size_t e = 0; e < m; ++e) pf[e] = fisher(lf, N, t, r.a[(size_t)el[e]], r.s[(size_t)el[e]]);
		bh_q(pf, q);
		for (size_t e = 0; e < m; ++e) {
			if (!(pf[e] <= o->max_p)) continue;
			const int32_t g = el[e];
			const int64_t a = r.a[(size_t)g], s = r.s[(size_t)g];
			const int64_t D = s * N - a * t, Vg = a * (N - a), Vt = (int64_t)t * (N - t);
			const double phi = (double)D / std::sqrt((double)Vg * (double)Vt);
			out += tr.name[ti], out += '\t', out += gene[(size_t)g];
			std::snprintf(b, sizeof(b), "\t%d\t%d\t%d\t%d\t%.4f\t%.3e\t%.3e\t", N, t, (int)a, (int)s, phi, pf[e], q[e]);
			out += b;
			if (o->n_perm > 0) std::snprintf(b, sizeof(b), "%d\t%.6f", r.k[(size_t)g], ((double)r.k[(size_t)g] + 1.0) / ((double)o->n_perm + 1.0));
			else std::snprintf(b, sizeof(b), "NA\tNA");
			out += b;
			if (o->lineage) { // `for` = the side the association points to; lf reaches N >= 2 pairs
				const int32_t *c = pc.data() + ((size_t)row_of[ti] * (size_t)G + (size_t)g) * 3;
				const int32_t n_for = D >= 0 ? c[1] : c[2], n_against = D >= 0 ? c[2] : c[1];
				std::snprintf(b, sizeof(b), "\t%d\t%d\t%d\t%.3e\t%.3e", c[0], c[1], c[2], binom_two_sided(lf, n_for, c[0]), binom_two_sided(lf, c[0] - n_against, c[0]));
				out += b;
			}
			out += '\n';
		}
	}
	ob.finish();
	report_time(route, G, A, tr.name.size(), o->n_perm, now_sec() - t_start);
	if (o->lineage) {
		int32_t rows = 0;
		for (const int32_t r : row_of) rows += r >= 0;
		report_lineage_time(rows, t_tree);
	}
	return 0;
}

// ---- quantitative traits ----

constexpr int32_t QTRAIT_MAX_COL = 32000; // the backend's limit (include/pangene_hip.h pga_pan_qtrait): |c2| <= 31 999 is two signed bytes

// The centred doubled midranks of v[N]: r2[c] = 2 #{v < v_c} + #{v == v_c} + 1, c2 = r2 - (N + 1); returns T = the sum over the tie
// groups of t^3 - t.  Doubles are compared as doubles, so -0.0 and 0.0 tie.
int64_t qtrait_ranks(const std::vector<double> &v, std::vector<int16_t> &c2)
{
	const int32_t N = (int32_t)v.size();
	c2.assign((size_t)N, 0);
	std::vector<int32_t> idx((size_t)N);
	std::iota(idx.begin(), idx.end(), 0);
	std::sort(idx.begin(), idx.end(), [&](int32_t x, int32_t y) { return v[(size_t)x] < v[(size_t)y]; });
	int64_t T = 0;
	for (int32_t b = 0; b < N;) {
		int32_t e = b + 1;
		while (e < N && v[(size_t)idx[(size_t)e]] == v[(size_t)idx[(size_t)b]]) ++e;
		const int64_t t = e - b;
		T += t * t * t - t;
		for (int32_t i = b; i < e; ++i) c2[(size_t)idx[(size_t)i]] = (int16_t)(2 * b + (e - b) + 1 - (N + 1));
		b = e;
	}
	return T;
}

// The backend's step on the host, by the definition: every permutation's value row from its order by indexing, every eligible gene's sum
// over its set bits, |D_p| >= |D|.  bits[G][W], c2[N]
void qtrait_host(const uint32_t *bits, const int16_t *c2, int32_t G, int32_t N, int32_t W, int32_t min_count, int32_t n, uint32_t seed,
                 std::vector<int32_t> &a, std::vector<int32_t> &d, std::vector<int32_t> &k)
{
	a.assign((size_t)G, 0), d.assign((size_t)G, 0), k.assign((size_t)G, 0);
	auto row_sum = [&](const uint32_t *b, const int16_t *val) {
		int64_t sum = 0;
		for (int32_t w = 0; w < W; ++w)
			for (uint32_t x = b[w]; x; x &= x - 1) sum += val[w * 32 + __builtin_ctz(x)];
		return sum;
	};
	std::vector<int32_t> el;
	for (int32_t g = 0; g < G; ++g) {
		const uint32_t *b = bits + (size_t)g * W;
		int32_t ca = 0;
		for (int32_t w = 0; w < W; ++w) ca += __builtin_popcount(b[w]);
		a[(size_t)g] = ca, d[(size_t)g] = (int32_t)row_sum(b, c2);
		if (std::min(ca, N - ca) >= min_count) el.push_back(g);
	}
	std::vector<int32_t> o;
	std::vector<int16_t> cp((size_t)N);
	for (int32_t p = 1; p <= n && !el.empty(); ++p) {
		make_order(N, seed, (uint32_t)p, o);
		for (int32_t r = 0; r < N; ++r) cp[(size_t)r] = c2[o[(size_t)r]];
		for (const int32_t g : el)
			if (std::llabs(row_sum(bits + (size_t)g * W, cp.data())) >= std::llabs((int64_t)d[(size_t)g])) ++k[(size_t)g];
	}
}

bool qopt_ok(const pg_qtrait_opt_t *o)
{
	return o != nullptr && o->n_perm >= 0 && o->n_perm <= TRAIT_MAX_PERM && o->min_count >= 1 && o->max_p == o->max_p;
}

// One trait over a presence matrix pres[G][A] (nonzero = present) and values val[A] (NaN = missing).  flat: N < 2 or one value only
struct QOne { int32_t N = 0; int64_t T = 0; bool flat = true; std::vector<int32_t> a, d, k; std::vector<uint8_t> elig; };

int qtrait_one(const uint8_t *pres, const double *val, int32_t G, int32_t A, const pg_qtrait_opt_t *o, QOne &r)
{
	std::vector<int32_t> col;
	std::vector<double> v;
	for (int32_t c = 0; c < A; ++c) {
		if (val[c] != val[c]) continue;
		if (!std::isfinite(val[c])) return PGA_ERR_ARG;
		col.push_back(c), v.push_back(val[c]);
	}
	const int32_t N = (int32_t)col.size(), W = (N + 31) / 32;
	r.N = N, r.T = 0, r.flat = true;
	r.a.assign((size_t)G, 0), r.d.assign((size_t)G, 0), r.k.assign((size_t)G, 0), r.elig.assign((size_t)G, 0);
	if (N > QTRAIT_MAX_COL) return PGA_ERR_RANGE;
	if (G > TRAIT_MAX_GENE) return PGA_ERR_RANGE;
	for (int32_t i = 1; i < N; ++i) if (v[(size_t)i] != v[0]) r.flat = false;
	if (r.flat) return 0; // nothing to test
	std::vector<int16_t> c2;
	r.T = qtrait_ranks(v, c2);
	std::vector<uint32_t> bits((size_t)G * W, 0);
	for (int32_t g = 0; g < G; ++g) {
		const uint8_t *row = pres + (size_t)g * A;
		uint32_t *b = bits.data() + (size_t)g * W;
		for (int32_t i = 0; i < N; ++i) if (row[col[(size_t)i]]) b[i >> 5] |= 1u << (i & 31);
	}
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	int rc = 0;
	if (be->pan_qtrait != nullptr) {
		const pga_qtrait_in_t in{bits.data(), c2.data(), G, N, o->min_count, o->n_perm, o->seed, nullptr, nullptr};
		pga_qtrait_out_t res{};
		rc = be->pan_qtrait(&in, &res);
		if (rc == 0) r.a.assign(res.a, res.a + (size_t)G), r.d.assign(res.d, res.d + (size_t)G), r.k.assign(res.k, res.k + (size_t)G);
	} else qtrait_host(bits.data(), c2.data(), G, N, W, o->min_count, o->n_perm, o->seed, r.a, r.d, r.k);
	t_count += now_sec() - t0;
	if (rc != 0) return rc;
	for (int32_t g = 0; g < G; ++g) r.elig[(size_t)g] = std::min(r.a[(size_t)g], N - r.a[(size_t)g]) >= o->min_count;
	return 0;
}

// every trait of tr over pres[G][A]: counts, statistics, lines.  0 or a PGA_ERR_* code; nothing is written unless every trait went through.
// z is the tie-corrected normal approximation of the rank sum WITHOUT continuity correction.
int qtrait_run(const char *route, const std::vector<std::string> &gene, const std::vector<uint8_t> &pres, int32_t A, const QTraits &tr, const pg_qtrait_opt_t *o,
               double t_start)
{
	if (!qopt_ok(o)) return PGA_ERR_ARG;
	const int32_t G = (int32_t)gene.size();
	t_count = 0;
	OutBuf ob;
	std::string &out = ob.s;
	out = "Trait\tGene\tN\tnG\tU\tauc\tz\tp_wilcox\tq_bh\tn_ge\tp_perm\n";
	char b[200];
	for (size_t ti = 0; ti < tr.name.size(); ++ti) {
		QOne r;
		const int rc = qtrait_one(pres.data(), tr.val.data() + ti * (size_t)A, G, A, o, r);
		if (rc != 0) return rc;
		const int32_t N = r.N;
		if (r.flat) { std::fprintf(stderr, "Note: trait %s has %s over its %d assemblies; skipped\n", tr.name[ti].c_str(), N < 2 ? "no two values" : "one value", N); continue; }
		std::vector<int32_t> el;
		for (int32_t g = 0; g < G; ++g) if (r.elig[(size_t)g]) el.push_back(g);
		const size_t m = el.size();
		const double tie = (double)(N + 1) - (double)r.T / ((double)N * (double)(N - 1));
		std::vector<double> z(m), pw(m), q;
		for (size_t e = 0; e < m; ++e) {
			const int64_t a = r.a[(size_t)el[e]];
			const double V = (double)(a * (N - a)) / 3.0 * tie;
			z[e] = (double)r.d[(size_t)el[e]] / std::sqrt(V);
			pw[e] = std::erfc(std::fabs(z[e]) / std::sqrt(2.0));
		}
		bh_q(pw, q);
		for (size_t e = 0; e < m; ++e) {
			if (!(pw[e] <= o->max_p)) continue;
			const int32_t g = el[e];
			const int64_t a = r.a[(size_t)g], D = r.d[(size_t)g], ab = a * (N - a);
			const double U = (double)(D + ab) * 0.5;
			out += tr.name[ti], out += '\t', out += gene[(size_t)g];
			std::snprintf(b, sizeof(b), "\t%d\t%d\t%.1f\t%.4f\t%.4f\t%.3e\t%.3e\t", N, (int)a, U, U / (double)ab, z[e], pw[e], q[e]);
			out += b;
			if (o->n_perm > 0) std::snprintf(b, sizeof(b), "%d\t%.6f", r.k[(size_t)g], ((double)r.k[(size_t)g] + 1.0) / ((double)o->n_perm + 1.0));
			else std::snprintf(b, sizeof(b), "NA\tNA");
			out += b, out += '\n';
		}
	}
	ob.finish();
	if (std::getenv("PANGENE_TRAIT_TIMING") != nullptr)
		std::fprintf(stderr, "[qtrait-timing] route=%s genes=%d assemblies=%d traits=%zu perms=%d count_ms=%.3f all_ms=%.3f\n", route, G, A, tr.name.size(), o->n_perm,
		             t_count * 1e3, (now_sec() - t_start) * 1e3);
	return 0;
}

// the gfa2matrix matrix (occurrences, [G][A]) -> presence bytes
void to_presence(const int32_t *mat, size_t n, std::vector<uint8_t> &pres)
{
	pres.resize(n);
	for (size_t i = 0; i < n; ++i) pres[i] = mat[i] > 0;
}

} // namespace
} // namespace pgx

using namespace pgx;

extern "C" {

void pg_trait_opt_init(pg_trait_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->n_perm = 1000, o->seed = 11, o->min_count = 1, o->max_p = 1.0;
}

int pg_trait_file(const char *gfa_fn, const char *trait_fn, const pg_trait_opt_t *o)
{
	const double t0 = now_sec();
	GfaMatrix m;
	if (gfa_matrix(gfa_fn, m) != 0) return cannot_open(gfa_fn);
	Traits tr;
	if (read_traits(trait_fn, m.asm_a, tr) != 0) return -3;
	std::vector<uint8_t> pres;
	to_presence(m.mat.data(), m.mat.size(), pres);
	const int rc = trait_run("file", m.seg, pres, (int32_t)m.asm_a.size(), tr, o, t0);
	if (rc != 0) { std::fprintf(stderr, "Error: pan_trait: %s\n", backend_default()->strerror(rc)); return -2; }
	return 0;
}

void pg_write_trait(pg_graph_t *q, const char *trait_fn, const pg_trait_opt_t *o)
{
	const double t0 = now_sec();
	std::vector<std::string> names, gene;
	std::vector<int32_t> mat;
	if (graph_matrix(q, names, mat) != 0) return;
	Traits tr;
	if (read_traits(trait_fn, names, tr) != 0) { set_error(PGA_ERR_ARG, "pg_write_trait: bad trait file"); return; }
	const int32_t G = q->n_seg;
	gene.reserve((size_t)G);
	for (int32_t i = 0; i < G; ++i) gene.emplace_back(q->d->gene[q->seg[i].gid].name);
	std::vector<uint8_t> pres;
	to_presence(mat.data(), mat.size(), pres);
	const int rc = trait_run("memory", gene, pres, (int32_t)names.size(), tr, o, t0);
	if (rc != 0) set_error(rc, "pg_write_trait");
}

int pg_pan_trait(const uint8_t *presence, const int8_t *labels, int32_t n_gene, int32_t n_asm, int32_t n_trait, const pg_trait_opt_t *o, int32_t *out)
{
	if (n_gene < 0 || n_asm < 0 || n_trait < 0 || !opt_ok(o)) return PGA_ERR_ARG;
	if (((size_t)n_gene * (size_t)n_asm > 0 && presence == nullptr) || ((size_t)n_trait * (size_t)n_asm > 0 && labels == nullptr)) return PGA_ERR_ARG;
	if ((size_t)n_trait * (size_t)n_gene > 0 && out == nullptr) return PGA_ERR_ARG;
	if (n_asm > TRAIT_MAX_COL) return PGA_ERR_RANGE;
	const size_t G = (size_t)n_gene, plane = (size_t)n_trait * G;
	for (int32_t ti = 0; ti < n_trait; ++ti) {
		One r;
		const int rc = trait_one(presence, labels + (size_t)ti * (size_t)n_asm, n_gene, n_asm, o, r);
		if (rc != 0) return rc;
		int32_t *p = out + (size_t)ti * G;
		for (size_t g = 0; g < G; ++g) {
			const bool e = r.elig[g] != 0;
			p[g] = r.N, p[plane + g] = r.t, p[2 * plane + g] = e ? r.a[g] : -1, p[3 * plane + g] = e ? r.s[g] : 0, p[4 * plane + g] = e ? r.k[g] : 0;
		}
	}
	return 0;
}

int pg_pan_pairs(const uint8_t *presence, const int8_t *labels, int32_t n_gene, int32_t n_asm, int32_t n_trait, const int64_t *rec, int32_t method, int32_t *out)
{
	if (n_gene < 0 || n_asm < 0 || n_trait < 0 || (method != PG_TREE_NJ && method != PG_TREE_UPGMA) || (n_asm >= 3 && rec == nullptr)) return PGA_ERR_ARG;
	if (((size_t)n_gene * (size_t)n_asm > 0 && presence == nullptr) || ((size_t)n_trait * (size_t)n_asm > 0 && labels == nullptr)) return PGA_ERR_ARG;
	if ((size_t)n_trait * (size_t)n_gene > 0 && out == nullptr) return PGA_ERR_ARG;
	std::vector<int32_t> pc;
	t_pairs = 0;
	const int rc = pairs_count(presence, labels, n_gene, n_asm, n_trait, rec, method, pc);
	if (rc != 0) return rc;
	const size_t plane = (size_t)n_trait * (size_t)n_gene;
	for (size_t i = 0; i < plane; ++i) out[i] = pc[3 * i], out[plane + i] = pc[3 * i + 1], out[2 * plane + i] = pc[3 * i + 2];
	return 0;
}

void pg_qtrait_opt_init(pg_qtrait_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->n_perm = 1000, o->seed = 11, o->min_count = 1, o->max_p = 1.0;
}

int pg_qtrait_file(const char *gfa_fn, const char *trait_fn, const pg_qtrait_opt_t *o)
{
	const double t0 = now_sec();
	GfaMatrix m;
	if (gfa_matrix(gfa_fn, m) != 0) return cannot_open(gfa_fn);
	QTraits tr;
	if (read_qtraits(trait_fn, m.asm_a, tr) != 0) return -3;
	std::vector<uint8_t> pres;
	to_presence(m.mat.data(), m.mat.size(), pres);
	const int rc = qtrait_run("file", m.seg, pres, (int32_t)m.asm_a.size(), tr, o, t0);
	if (rc != 0) { std::fprintf(stderr, "Error: pan_qtrait: %s\n", backend_default()->strerror(rc)); return -2; }
	return 0;
}

void pg_write_qtrait(pg_graph_t *q, const char *trait_fn, const pg_qtrait_opt_t *o)
{
	const double t0 = now_sec();
	std::vector<std::string> names, gene;
	std::vector<int32_t> mat;
	if (graph_matrix(q, names, mat) != 0) return;
	QTraits tr;
	if (read_qtraits(trait_fn, names, tr) != 0) { set_error(PGA_ERR_ARG, "pg_write_qtrait: bad trait file"); return; }
	const int32_t G = q->n_seg;
	gene.reserve((size_t)G);
	for (int32_t i = 0; i < G; ++i) gene.emplace_back(q->d->gene[q->seg[i].gid].name);
	std::vector<uint8_t> pres;
	to_presence(mat.data(), mat.size(), pres);
	const int rc = qtrait_run("memory", gene, pres, (int32_t)names.size(), tr, o, t0);
	if (rc != 0) set_error(rc, "pg_write_qtrait");
}

int pg_pan_qtrait(const uint8_t *presence, const double *values, int32_t n_gene, int32_t n_asm, int32_t n_trait, const pg_qtrait_opt_t *o, int32_t *out)
{
	if (n_gene < 0 || n_asm < 0 || n_trait < 0 || !qopt_ok(o)) return PGA_ERR_ARG;
	if (((size_t)n_gene * (size_t)n_asm > 0 && presence == nullptr) || ((size_t)n_trait * (size_t)n_asm > 0 && values == nullptr)) return PGA_ERR_ARG;
	if ((size_t)n_trait * (size_t)n_gene > 0 && out == nullptr) return PGA_ERR_ARG;
	const size_t G = (size_t)n_gene, plane = (size_t)n_trait * G;
	for (int32_t ti = 0; ti < n_trait; ++ti) {
		QOne r;
		const int rc = qtrait_one(presence, values + (size_t)ti * (size_t)n_asm, n_gene, n_asm, o, r);
		if (rc != 0) return rc;
		int32_t *p = out + (size_t)ti * G;
		for (size_t g = 0; g < G; ++g) {
			const bool e = r.elig[g] != 0;
			p[g] = r.N, p[plane + g] = e ? r.a[g] : -1, p[2 * plane + g] = e ? r.d[g] : 0, p[3 * plane + g] = e ? r.k[g] : 0;
		}
	}
	return 0;
}

} // extern "C"
