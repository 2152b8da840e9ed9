// trait.cpp -- gene-trait association (pg_trait_file, pg_write_trait, pg_pan_trait; include/pangene_amd.h): which genes go with a
// binary phenotype of the assemblies.  Per trait the columns that have a value are compacted and every gene becomes a bit row over
// them; the observed counts and the label-permutation counts k_g come from the backend (pga_pan_trait: the permuted label rows are
// made and counted on the device and one integer per gene comes back), or from the plain loops below when the backend has no such
// entry.  Everything the permutation test decides is an integer; phi, the Fisher p and the Benjamini-Hochberg q are computed here,
// for printing only, by code both builds share.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>
#include "pg_internal.hpp"

namespace pgx {
namespace {

constexpr int32_t TRAIT_MAX_COL = 16777215, TRAIT_MAX_GENE = 16777215, TRAIT_MAX_PERM = 2147483646;

uint64_t mix64(uint64_t z) // splitmix64's output function (as curves.cpp)
{
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

// order p >= 1 of N columns: make_orders' sequence (curves.cpp)
void make_order(int32_t N, uint32_t seed, uint32_t p, std::vector<int32_t> &o)
{
	o.resize((size_t)N);
	for (int32_t i = 0; i < N; ++i) o[(size_t)i] = i;
	uint64_t x = mix64((uint64_t)seed << 32 | (uint64_t)p);
	for (int32_t i = N - 1; i >= 1; --i) {
		x += 0x9E3779B97F4A7C15ull;
		const uint64_t j = mix64(x) % (uint64_t)(i + 1);
		std::swap(o[(size_t)i], o[(size_t)j]);
	}
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

bool opt_ok(const pg_trait_opt_t *o) { return o != nullptr && o->n_perm >= 0 && o->n_perm <= TRAIT_MAX_PERM && o->min_count >= 1 && o->max_p == o->max_p; }

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

struct Traits { std::vector<std::string> name; std::vector<int8_t> lab; }; // lab[T][A]

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

// 0, or -1 with a message (the line number in it) on stderr
int read_traits(const char *fn, const std::vector<std::string> &asm_name, Traits &tr)
{
	std::vector<std::string> lines;
	if (fn == nullptr || read_lines(fn, lines) != 0) { std::fprintf(stderr, "Error: cannot open trait file %s\n", fn ? fn : "(null)"); return -1; }
	if (lines.empty()) { std::fprintf(stderr, "Error: %s: line 1: no header line\n", fn); return -1; }
	const std::vector<std::string> h = split_tab(lines[0]);
	const size_t T = h.size() - 1, A = asm_name.size();
	tr.name.assign(h.begin() + 1, h.end());
	tr.lab.assign(T * A, (int8_t)-1);
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
		for (size_t j = 0; j < T; ++j) {
			const std::string &v = f[j + 1];
			int8_t x;
			if (v == "1") x = 1; else if (v == "0") x = 0; else if (v == "NA" || v.empty()) x = -1;
			else { std::fprintf(stderr, "Error: %s: line %zu: value %s is not 1, 0 or NA\n", fn, ln + 1, v.c_str()); return -1; }
			tr.lab[j * A + (size_t)it->second] = x;
		}
	}
	return 0;
}

// PANGENE_TRAIT_TIMING=1: one line on stderr per call
void report_time(const char *route, int32_t G, int32_t A, size_t T, int32_t n, double t_all)
{
	if (std::getenv("PANGENE_TRAIT_TIMING") == nullptr) return;
	std::fprintf(stderr, "[trait-timing] route=%s genes=%d assemblies=%d traits=%zu perms=%d count_ms=%.3f all_ms=%.3f\n", route, G, A, T, n, t_count * 1e3, t_all * 1e3);
}

// every trait of tr over pres[G][A]: counts, statistics, lines.  0 or a PGA_ERR_* code; nothing is written unless every trait went through
int trait_run(const char *route, const std::vector<std::string> &gene, const std::vector<uint8_t> &pres, int32_t A, const Traits &tr, const pg_trait_opt_t *o,
              double t_start)
{
	if (!opt_ok(o)) return PGA_ERR_ARG;
	if (A > TRAIT_MAX_COL) return PGA_ERR_RANGE;
	const int32_t G = (int32_t)gene.size();
	t_count = 0;
	std::string out = "Trait\tGene\tN\tnT\tnG\tnTG\tphi\tp_fisher\tq_bh\tn_ge\tp_perm\n";
	char b[160];
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
		std::vector<double> pf(m), q(m);
		for (size_t e = 0; e < m; ++e) pf[e] = fisher(lf, N, t, r.a[(size_t)el[e]], r.s[(size_t)el[e]]);
		std::vector<size_t> idx(m);
		std::iota(idx.begin(), idx.end(), (size_t)0);
		std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return pf[x] < pf[y]; }); // ties by row
		double run = 1.0;
		for (size_t j = m; j >= 1; --j) {
			run = std::min(run, pf[idx[j - 1]] * (double)m / (double)j);
			q[idx[j - 1]] = run;
		}
		for (size_t e = 0; e < m; ++e) {
			if (!(pf[e] <= o->max_p)) continue;
			const int32_t g = el[e];
			const int64_t a = r.a[(size_t)g], s = r.s[(size_t)g];
			const int64_t D = s * N - a * t, Vg = a * (N - a), Vt = (int64_t)t * (N - t);
			const double phi = (double)D / std::sqrt((double)Vg * (double)Vt);
			out += tr.name[ti], out += '\t', out += gene[(size_t)g];
			std::snprintf(b, sizeof(b), "\t%d\t%d\t%d\t%d\t%.4f\t%.3e\t%.3e\t", N, t, (int)a, (int)s, phi, pf[e], q[e]);
			out += b;
			if (o->n_perm > 0) std::snprintf(b, sizeof(b), "%d\t%.6f\n", r.k[(size_t)g], ((double)r.k[(size_t)g] + 1.0) / ((double)o->n_perm + 1.0));
			else std::snprintf(b, sizeof(b), "NA\tNA\n");
			out += b;
		}
	}
	FILE *fp = out_stream();
	std::fwrite(out.data(), 1, out.size(), fp);
	std::fflush(fp);
	report_time(route, G, A, tr.name.size(), o->n_perm, now_sec() - t_start);
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
	if (gfa_matrix(gfa_fn, m) != 0) { std::fprintf(stderr, "Error: cannot open %s\n", gfa_fn ? gfa_fn : "-"); return -1; }
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

} // extern "C"
