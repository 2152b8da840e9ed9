// curves.cpp -- pangenome accumulation curves (pg_curves_file, pg_write_curves, pg_pan_curves; include/pangene_amd.h): pan, core,
// new and unique genes as the assemblies of a gene x assembly presence matrix are added in n orders.  The matrix is the one
// gfa2matrix prints (the graph in memory: the backend's gene_matrix; a GFA file: the gfa2matrix reader), the counting runs on the
// backend (pga_pan_curves), or as the plain loops below when the backend has no such entry.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "pg_internal.hpp"

namespace pgx {
namespace {

// order 0: the columns as they are; order p >= 1: fisher_yates_order
void make_orders(int32_t A, int32_t n, uint32_t seed, std::vector<int32_t> &ord)
{
	ord.resize((size_t)n * (size_t)A);
	for (int32_t p = 0; p < n; ++p) {
		int32_t *o = ord.data() + (size_t)p * A;
		if (p == 0) for (int32_t i = 0; i < A; ++i) o[i] = i;
		else fisher_yates_order(A, seed, (uint32_t)p, o);
	}
}

// The backend's step on the host: per order and gene the ranks f1 (first present column), f2 (second) and z (first absent column),
// A where there is none, from the gene's present (absent) columns or by walking the order, whichever is shorter; then the curves
// from the three histograms.  out[4][n][A]
void curves_host(const uint32_t *bits, const int32_t *ord, int32_t G, int32_t A, int32_t n, int32_t *out)
{
	const int32_t W = (A + 31) / 32;
	const size_t plane = (size_t)n * A;
	std::memset(out, 0, sizeof(int32_t) * 4 * plane);
	if (A == 0 || n == 0) return;
	auto has = [&](int32_t g, int32_t j) { return (bits[(size_t)g * W + (size_t)(j >> 5)] >> (j & 31)) & 1u; };
	std::vector<int32_t> cnt((size_t)G), off((size_t)G + 1, 0), cols;
	const int32_t T = std::max<int32_t>(2, (int32_t)std::ceil(std::sqrt(2.0 * A)));
	for (int32_t g = 0; g < G; ++g) { // a gene's list: its present columns or its absent ones, where that is the short side
		int32_t c = 0;
		for (int32_t j = 0; j < A; ++j) c += (int32_t)has(g, j);
		cnt[(size_t)g] = c;
		const bool pres = c <= A - c;
		if ((pres ? c : A - c) <= T)
			for (int32_t j = 0; j < A; ++j) if ((bool)has(g, j) == pres) cols.push_back(j);
		off[(size_t)g + 1] = (int32_t)cols.size();
	}
	std::vector<int32_t> rank((size_t)A), h1((size_t)A + 1), h2((size_t)A + 1), hz((size_t)A + 1);
	for (int32_t p = 0; p < n; ++p) {
		const int32_t *o = ord + (size_t)p * A;
		for (int32_t i = 0; i < A; ++i) rank[(size_t)o[i]] = i;
		std::fill(h1.begin(), h1.end(), 0), std::fill(h2.begin(), h2.end(), 0), std::fill(hz.begin(), hz.end(), 0);
		for (int32_t g = 0; g < G; ++g) {
			const int32_t c = cnt[(size_t)g], L = off[(size_t)g + 1] - off[(size_t)g];
			const int32_t *lst = cols.data() + off[(size_t)g];
			const bool pres_list = L > 0 && c <= A - c, abs_list = L > 0 && !pres_list;
			int32_t f1 = A, f2 = A, z = A;
			if (pres_list) {
				for (int32_t i = 0; i < L; ++i) { const int32_t r = rank[(size_t)lst[i]]; if (r < f1) f2 = f1, f1 = r; else if (r < f2) f2 = r; }
			} else if (c > 0) {
				for (int32_t r = 0; r < A; ++r) if (has(g, o[r])) { if (f1 == A) f1 = r; else { f2 = r; break; } }
			}
			if (abs_list) {
				for (int32_t i = 0; i < L; ++i) z = std::min(z, rank[(size_t)lst[i]]);
			} else if (c < A) {
				for (int32_t r = 0; r < A; ++r) if (!has(g, o[r])) { z = r; break; }
			}
			++h1[(size_t)f1], ++h2[(size_t)f2], ++hz[(size_t)z];
		}
		int32_t c1 = 0, c2 = 0, cz = 0;
		for (int32_t i = 0; i < A; ++i) {
			c1 += h1[(size_t)i], c2 += h2[(size_t)i], cz += hz[(size_t)i];
			const size_t at = (size_t)p * A + (size_t)i;
			out[at] = c1, out[plane + at] = G - cz, out[2 * plane + at] = h1[(size_t)i], out[3 * plane + at] = c1 - c2;
		}
	}
}

double t_count = 0; // seconds of the last count step (backend or host loops)

// bits[G][(A + 31) / 32] -> out[4][n][A]; 0 or a PGA_ERR_* code
int curves_count(const std::vector<uint32_t> &bits, int32_t G, int32_t A, const pg_curves_opt_t *o, std::vector<int32_t> &out)
{
	const int32_t n = o->n_perm;
	if (G < 0 || A < 0 || n < 0) return PGA_ERR_ARG;
	std::vector<int32_t> ord;
	make_orders(A, n, o->seed, ord);
	out.assign((size_t)4 * n * A, 0);
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	if (be->pan_curves != nullptr) {
		const pga_curves_in_t in{bits.data(), ord.data(), G, A, n};
		pga_curves_out_t res{};
		const int rc = be->pan_curves(&in, &res);
		if (rc != 0) return rc;
		if (!out.empty()) std::memcpy(out.data(), res.count, sizeof(int32_t) * out.size());
	} else curves_host(bits.data(), ord.data(), G, A, n, out.data());
	t_count = now_sec() - t0;
	return 0;
}

void put_row(std::string &s, const char *stat, int32_t p, const int32_t *v, int32_t A)
{
	char b[16];
	s += stat, s += '\t', s += std::to_string(p);
	for (int32_t i = 0; i < A; ++i) { std::snprintf(b, sizeof(b), "\t%d", v[i]); s += b; }
	s += '\n';
}

void print_curves(const std::vector<int32_t> &out, int32_t A, int32_t n)
{
	OutBuf ob;
	std::string &s = ob.s;
	s = "Stat\tPerm";
	for (int32_t i = 1; i <= A; ++i) s += '\t', s += std::to_string(i);
	s += '\n';
	static const char *const name[4] = { "pan", "core", "new", "unique" };
	for (int st = 0; st < 4; ++st)
		for (int32_t p = 0; p < n; ++p) {
			put_row(s, name[st], p, out.data() + ((size_t)st * n + p) * A, A);
			ob.flush_if_full();
		}
	ob.finish();
}

// PANGENE_CURVES_TIMING=1: one line on stderr per call (tests/run_curves_timing.py reads it)
void report_time(const char *route, int32_t G, int32_t A, int32_t n, double t_prep, double t_write)
{
	if (std::getenv("PANGENE_CURVES_TIMING") == nullptr) return;
	std::fprintf(stderr, "[curves-timing] route=%s genes=%d assemblies=%d orders=%d prep_ms=%.3f count_ms=%.3f write_ms=%.3f\n", route, G, A, n,
	             t_prep * 1e3, t_count * 1e3, t_write * 1e3);
}

int curves_run(const char *route, const int32_t *mat, int32_t G, int32_t A, const pg_curves_opt_t *o, double t_start)
{
	std::vector<uint32_t> bits;
	pack_rows(mat, G, A, bits); // matrix entries > 0 = present
	std::vector<int32_t> out;
	const double t_prep = now_sec() - t_start;
	const int rc = curves_count(bits, G, A, o, out);
	if (rc != 0) return rc;
	const double t1 = now_sec();
	print_curves(out, A, o->n_perm);
	report_time(route, G, A, o->n_perm, t_prep, now_sec() - t1);
	return 0;
}

} // namespace
} // namespace pgx

using namespace pgx;

extern "C" {

void pg_curves_opt_init(pg_curves_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->n_perm = 10, o->seed = 11;
}

int pg_curves_file(const char *gfa_fn, const pg_curves_opt_t *o)
{
	const double t0 = now_sec();
	GfaMatrix m;
	if (gfa_matrix(gfa_fn, m) != 0) return cannot_open(gfa_fn);
	const int rc = curves_run("file", m.mat.data(), (int32_t)m.seg.size(), (int32_t)m.asm_a.size(), o, t0);
	if (rc != 0) { std::fprintf(stderr, "Error: pan_curves: %s\n", backend_default()->strerror(rc)); return -2; }
	return 0;
}

void pg_write_curves(pg_graph_t *q, const pg_curves_opt_t *o)
{
	const double t0 = now_sec();
	std::vector<std::string> names;
	std::vector<int32_t> mat;
	if (graph_matrix(q, names, mat) != 0) return;
	const int rc = curves_run("memory", mat.data(), q->n_seg, (int32_t)names.size(), o, t0);
	if (rc != 0) set_error(rc, "pg_write_curves");
}

int pg_pan_curves(const uint8_t *presence, int32_t n_gene, int32_t n_asm, const pg_curves_opt_t *o, int32_t *out)
{
	if (n_gene < 0 || n_asm < 0 || o == nullptr || o->n_perm < 0) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_rows(presence, n_gene, n_asm, bits);
	std::vector<int32_t> res;
	const int rc = curves_count(bits, n_gene, n_asm, o, res);
	if (rc == 0 && !res.empty()) std::memcpy(out, res.data(), sizeof(int32_t) * res.size());
	return rc;
}

} // extern "C"
