// assoc.cpp -- gene associations (pg_assoc_file, pg_write_assoc, pg_pan_assoc; include/pangene_amd.h): the gene pairs whose presence
// over the assemblies is correlated (phi) or anti-correlated.  Every gene is a bit row over the assemblies; the pairs are counted and
// selected on the backend (pga_pan_assoc: the selection happens on the device and a sparse list comes back), or by the plain loops
// below when the backend has no such entry.  The selection is integer arithmetic in both; phi is computed here, for printing only.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "pg_internal.hpp"

namespace pgx {
namespace {

constexpr int32_t ASSOC_MAX_ASM = 16777215;

typedef unsigned __int128 u128;

// 10^6 D^2 >= p^2 V_g V_h and the sign of D: the definition.  |D| < 2^46, V < 2^46, p <= 1000: both sides < 2^112
inline bool selected(int64_t D, int64_t Vg, int64_t Vh, int32_t p, int32_t sign)
{
	if (sign == PG_ASSOC_POS && D < 0) return false;
	if (sign == PG_ASSOC_NEG && D >= 0) return false;
	const u128 d = (u128)(uint64_t)(D < 0 ? -D : D);
	return d * d * (u128)1000000u >= (u128)(uint64_t)Vg * (u128)(uint64_t)Vh * (u128)((uint32_t)p * (uint32_t)p);
}

// The backend's step on the host.  bits[G][W]; pairs in ascending (g, h) as they are found.  Returns the number selected; only the
// first max_pair are kept.
int64_t assoc_host(const uint32_t *bits, int32_t G, int32_t A, int32_t W, int32_t min_count, int32_t p, int32_t sign, int64_t max_pair,
                   std::vector<int32_t> &count, std::vector<int32_t> &pair)
{
	count.assign((size_t)G, 0);
	std::vector<int32_t> el; // eligible rows
	for (int32_t g = 0; g < G; ++g) {
		int32_t a = 0;
		for (int32_t k = 0; k < W; ++k) a += __builtin_popcount(bits[(size_t)g * W + k]);
		count[(size_t)g] = a;
		if (std::min(a, A - a) >= min_count) el.push_back(g);
	}
	int64_t n = 0;
	pair.clear();
	for (size_t i = 0; i < el.size(); ++i) {
		const uint32_t *bi = bits + (size_t)el[i] * W;
		const int64_t a = count[(size_t)el[i]], Vg = a * (A - a);
		for (size_t j = i + 1; j < el.size(); ++j) {
			const uint32_t *bj = bits + (size_t)el[j] * W;
			int32_t s = 0;
			for (int32_t k = 0; k < W; ++k) s += __builtin_popcount(bi[k] & bj[k]);
			const int64_t b = count[(size_t)el[j]];
			if (!selected((int64_t)s * A - a * b, Vg, b * (A - b), p, sign)) continue;
			if (n++ < max_pair) pair.push_back(el[i]), pair.push_back(el[j]), pair.push_back(s);
		}
	}
	return n;
}

double t_count = 0; // seconds of the last selection step (backend or host loops)

struct Result { int64_t n = 0; std::vector<int32_t> count, own; const int32_t *pair = nullptr; }; // pair[n][3]

// 0, or a PGA_ERR_* code; r.n is the number of selected pairs in both cases where it is known
int assoc_select(const std::vector<uint32_t> &bits, int32_t G, int32_t A, const pg_assoc_opt_t *o, Result &r)
{
	r.n = 0, r.pair = nullptr;
	if (G < 0 || A < 0 || o == nullptr) return PGA_ERR_ARG;
	if (!(o->min_phi >= 0.0 && o->min_phi <= 1.0) || o->min_count < 1 || o->sign < PG_ASSOC_BOTH || o->sign > PG_ASSOC_NEG || o->max_pair < 0) return PGA_ERR_ARG;
	if (A > ASSOC_MAX_ASM) return PGA_ERR_RANGE;
	const int32_t p = (int32_t)std::floor(1000.0 * o->min_phi + 0.5);
	const int32_t W = (A + 31) / 32;
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	int rc = 0;
	if (be->pan_assoc != nullptr) {
		const pga_assoc_in_t in{bits.data(), G, A, o->min_count, p, o->sign, o->max_pair};
		pga_assoc_out_t res{};
		rc = be->pan_assoc(&in, &res);
		r.n = res.n_pair;
		if (rc == 0) {
			r.pair = res.pair;
			r.count.assign(res.count, res.count + (size_t)G);
		}
	} else {
		r.n = assoc_host(bits.data(), G, A, W, o->min_count, p, o->sign, o->max_pair, r.count, r.own);
		r.pair = r.own.data();
		if (r.n > o->max_pair) rc = PGA_ERR_RANGE;
	}
	t_count = now_sec() - t0;
	if (rc == PGA_ERR_RANGE && r.n > o->max_pair)
		std::fprintf(stderr, "Error: %lld gene pairs passed, more than the %lld allowed (-x); raise -r or -c\n", (long long)r.n, (long long)o->max_pair);
	return rc;
}

void print_assoc(const std::vector<std::string> &gene, int32_t A, const Result &r)
{
	OutBuf ob;
	std::string &s = ob.s;
	s = "GeneA\tGeneB\tnA\tnB\tnAB\tphi\n";
	char b[96];
	for (int64_t i = 0; i < r.n; ++i) {
		const int32_t g = r.pair[i * 3], h = r.pair[i * 3 + 1], x = r.pair[i * 3 + 2];
		const int64_t na = r.count[(size_t)g], nb = r.count[(size_t)h];
		const int64_t D = (int64_t)x * A - na * nb, Vg = na * (A - na), Vh = nb * (A - nb);
		const double phi = (double)D / std::sqrt((double)Vg * (double)Vh);
		s += gene[(size_t)g], s += '\t', s += gene[(size_t)h];
		std::snprintf(b, sizeof(b), "\t%d\t%d\t%d\t%.4f\n", (int)na, (int)nb, (int)x, phi);
		s += b;
		ob.flush_if_full();
	}
	ob.finish();
}

// PANGENE_ASSOC_TIMING=1: one line on stderr per call
void report_time(const char *route, int32_t G, int32_t A, int64_t n, double t_prep, double t_write)
{
	if (std::getenv("PANGENE_ASSOC_TIMING") == nullptr) return;
	std::fprintf(stderr, "[assoc-timing] route=%s genes=%d assemblies=%d pairs=%lld prep_ms=%.3f select_ms=%.3f write_ms=%.3f\n", route, G, A,
	             (long long)n, t_prep * 1e3, t_count * 1e3, t_write * 1e3);
}

int assoc_run(const char *route, const std::vector<std::string> &gene, const std::vector<uint32_t> &bits, int32_t A, const pg_assoc_opt_t *o,
              double t_start)
{
	Result r;
	const double t_prep = now_sec() - t_start;
	const int rc = assoc_select(bits, (int32_t)gene.size(), A, o, r);
	if (rc != 0) return rc;
	const double t1 = now_sec();
	print_assoc(gene, A, r);
	report_time(route, (int32_t)gene.size(), A, r.n, t_prep, now_sec() - t1);
	return 0;
}

} // namespace
} // namespace pgx

using namespace pgx;

extern "C" {

void pg_assoc_opt_init(pg_assoc_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->min_phi = 0.8, o->min_count = 2, o->sign = PG_ASSOC_BOTH, o->max_pair = 16777216;
}

int pg_assoc_file(const char *gfa_fn, const pg_assoc_opt_t *o)
{
	const double t0 = now_sec();
	GfaMatrix m;
	if (gfa_matrix(gfa_fn, m) != 0) return cannot_open(gfa_fn);
	const int32_t A = (int32_t)m.asm_a.size(), G = (int32_t)m.seg.size();
	std::vector<uint32_t> bits;
	pack_rows(m.mat.data(), G, A, bits); // the gfa2matrix matrix: gene g is in assembly a when its entry is > 0
	const int rc = assoc_run("file", m.seg, bits, A, o, t0);
	if (rc != 0) { std::fprintf(stderr, "Error: pan_assoc: %s\n", backend_default()->strerror(rc)); return -2; }
	return 0;
}

void pg_write_assoc(pg_graph_t *q, const pg_assoc_opt_t *o)
{
	const double t0 = now_sec();
	std::vector<std::string> names, gene;
	std::vector<int32_t> mat;
	if (graph_matrix(q, names, mat) != 0) return;
	const int32_t G = q->n_seg, A = (int32_t)names.size();
	gene.reserve((size_t)G);
	for (int32_t i = 0; i < G; ++i) gene.emplace_back(q->d->gene[q->seg[i].gid].name);
	std::vector<uint32_t> bits;
	pack_rows(mat.data(), G, A, bits);
	const int rc = assoc_run("memory", gene, bits, A, o, t0);
	if (rc != 0) set_error(rc, "pg_write_assoc");
}

int64_t pg_pan_assoc(const uint8_t *presence, int32_t n_gene, int32_t n_asm, const pg_assoc_opt_t *o, int32_t *pair, int64_t cap)
{
	if (n_gene < 0 || n_asm < 0 || cap < 0 || ((size_t)n_gene * (size_t)n_asm > 0 && presence == nullptr) || (cap > 0 && pair == nullptr)) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_rows(presence, n_gene, n_asm, bits);
	Result r;
	const int rc = assoc_select(bits, n_gene, n_asm, o, r);
	if (rc != 0) return rc;
	const int64_t n = r.n < cap ? r.n : cap;
	if (n > 0) std::memcpy(pair, r.pair, sizeof(int32_t) * 3 * (size_t)n);
	return r.n;
}

} // extern "C"
