// pan_permanova.hpp -- PERMANOVA (pg_permanova_file, pg_write_permanova, pg_pan_permanova, pg_pan_permanova_presence, pangene permanova;
// DESIGN.md section 8 "PERMANOVA"): the trait file by trait.cpp's reader; per trait the compacted submatrix of the fixed-point distances
// of pan_tree.hpp, its scaling, and T, A, B of the observed labels and the permutation count k from the backend (pga_pan_permanova) or
// from the plain loops below; the statistics and the text are code both builds share.

namespace pgx {
namespace {

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

// the items and the trait file, the distances, then one line per trait; nothing is written unless every trait went through
int permanova_run(const ItemSource &src, const char *trait_fn, const pg_permanova_opt_t *o)
{
	const double t_start = now_sec();
	std::vector<std::string> names;
	std::vector<uint32_t> bits;
	int32_t M;
	if (src(o->type, names, bits, M) != 0) return PAN_NO_ITEMS;
	Traits tr;
	if (read_traits(trait_fn, names, tr) != 0) return PAN_BAD_FILE;
	const int32_t A = (int32_t)names.size();
	if (!perma_opt_ok(o)) return PGA_ERR_ARG;
	const double t_prep = now_sec() - t_start;
	std::vector<int32_t> q;
	int32_t F = 20;
	if (const int rc = fixed_dist(bits, M, A, o->metric, q, &F)) return rc;
	t_perma = 0;
	OutBuf ob;
	std::string &s = ob.s;
	s = "Trait\tN\tn1\tn0\tFbits\tSS_total\tSS_within\tF\tR2\tn_ge\tp_perm\n";
	char b[256];
	for (size_t ti = 0; ti < tr.name.size(); ++ti) {
		Perma r;
		const int rc = permanova_one(q.data(), A, tr.lab.data() + ti * (size_t)A, F, o->n_perm, o->seed, r);
		if (rc != 0) return rc;
		if (r.skip) {
			std::fprintf(stderr, "Note: trait %s has %s over its %d assemblies; skipped\n", tr.name[ti].c_str(),
			             r.skip == 2 ? "no distance above zero" : r.N < 3 ? "fewer than 3 values" : "one group only", r.N);
			continue;
		}
		const int64_t N = r.N, n1 = r.n1, n0 = N - n1;
		const i128 X = (i128)N * r.A - (i128)(2 * n1) * r.B + (i128)n1 * r.T; // 2 n0 n1 SSW
		const i128 tn = (i128)r.T * (n0 * n1), Y = tn - (i128)N * X;          // 2 N n0 n1 (SST - SSW)
		std::snprintf(b, sizeof(b), "\t%d\t%d\t%d\t%d\t%.6f\t%.6f\t", (int)N, (int)n1, (int)n0, r.Fe, ratio(r.T, 2 * N, 2 * r.Fe), ratio(X, 2 * n0 * n1, 2 * r.Fe));
		s += tr.name[ti], s += b;
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
		std::fprintf(stderr, "[permanova-timing] route=%s items=%d assemblies=%d traits=%zu perms=%d prep_ms=%.3f stat_ms=%.3f all_ms=%.3f\n", src.route(), M, A, tr.name.size(),
		             o->n_perm, t_prep * 1e3, t_perma * 1e3, (now_sec() - t_start) * 1e3);
	return 0;
}

} // namespace
} // namespace pgx

extern "C" {

void pg_permanova_opt_init(pg_permanova_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->n_perm = 1000, o->seed = 11, o->frac_bits = 20;
}

int pg_permanova_file(const char *gfa_fn, const char *trait_fn, const pg_permanova_opt_t *o)
{
	if (o == nullptr) { std::fprintf(stderr, "Error: pan_permanova: no options\n"); return -2; }
	return file_result(permanova_run(items_of_file(gfa_fn), trait_fn, o), gfa_fn, "pan_permanova");
}

void pg_write_permanova(pg_graph_t *q, const char *trait_fn, const pg_permanova_opt_t *o)
{
	if (o == nullptr) { set_error(PGA_ERR_ARG, "pg_write_permanova"); return; }
	graph_result(permanova_run(items_of_graph(q), trait_fn, o), "pg_write_permanova", "pg_write_permanova: bad trait file");
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
	std::vector<int32_t> q;
	*frac_bits = 20;
	if (const int rc = fixed_dist(bits, n_item, n_asm, o->metric, q, frac_bits)) return rc;
	return permanova_rows(q.data(), n_asm, labels, n_trait, *frac_bits, o, out);
}

} // extern "C"
