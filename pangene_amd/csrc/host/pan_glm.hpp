// pan_glm.hpp -- gene-trait tests adjusted for population structure (pg_glm_file, pg_write_glm, pg_pan_glm, pangene glm; DESIGN.md
// section 8 "Structure-adjusted association"): the Rao score test of every gene against a trait, with the principal coordinates of
// pan_pcoa.hpp as covariates.  The trait files come from trait.cpp's readers, the axes from pcoa_core.  Per trait ONE null fit on the
// host in fp64 (logistic by Newton/IRLS, or least squares); then per gene four numbers -- a, U, V, s_w -- from the backend (pga_pan_glm:
// the presence bits times 16 columns a trait on the fp64 matrix cores, then a forward substitution) or, when the backend has no such
// entry, from the second implementation below, which walks the set bits.  The null fit, Beta, SE, Z, p, q, lambda and the text are
// code both builds share.  Floating point: two builds agree within the tolerances of DESIGN.md, not byte for byte.

namespace pgx {
namespace {

constexpr int32_t GLM_MAX_COL = 16384, GLM_MAX_COV = 13, GLM_COLS = 16; // the backend's limits and layout (include/pangene_hip.h pga_pan_glm)
constexpr int32_t GLM_MAX_ITER = 30, GLM_MAX_HALVE = 10;
constexpr double GLM_STEP = 1e-9, GLM_LL_NOISE = 1e-10, GLM_ETA = 30.0, GLM_PIVOT = 1e-12, GLM_COLLINEAR = 1e-8, GLM_CHI2_MEDIAN = 0.4549364;

// Cholesky of the symmetric n x n matrix H (row-major) in place: the lower triangle becomes L, the upper one zero.  false when a pivot
// is not above GLM_PIVOT times its diagonal entry (a NaN fails too)
bool glm_chol(std::vector<double> &H, int32_t n)
{
	for (int32_t j = 0; j < n; ++j) {
		const double d0 = H[(size_t)(j * n + j)];
		double d = d0;
		for (int32_t p = 0; p < j; ++p) d -= H[(size_t)(j * n + p)] * H[(size_t)(j * n + p)];
		if (!(d > GLM_PIVOT * d0)) return false;
		H[(size_t)(j * n + j)] = std::sqrt(d);
		for (int32_t i = j + 1; i < n; ++i) {
			double s = H[(size_t)(i * n + j)];
			for (int32_t p = 0; p < j; ++p) s -= H[(size_t)(i * n + p)] * H[(size_t)(j * n + p)];
			H[(size_t)(i * n + j)] = s / H[(size_t)(j * n + j)];
		}
	}
	for (int32_t i = 0; i < n; ++i)
		for (int32_t j = i + 1; j < n; ++j) H[(size_t)(i * n + j)] = 0.0;
	return true;
}

// x = (L L')^-1 b, in place
void glm_solve(const std::vector<double> &L, int32_t n, std::vector<double> &b)
{
	for (int32_t i = 0; i < n; ++i) {
		for (int32_t j = 0; j < i; ++j) b[(size_t)i] -= L[(size_t)(i * n + j)] * b[(size_t)j];
		b[(size_t)i] /= L[(size_t)(i * n + i)];
	}
	for (int32_t i = n - 1; i >= 0; --i) {
		for (int32_t j = i + 1; j < n; ++j) b[(size_t)i] -= L[(size_t)(j * n + i)] * b[(size_t)j];
		b[(size_t)i] /= L[(size_t)(i * n + i)];
	}
}

// What the null fit of one trait leaves.  skip: 0 = fitted or tried, 1 = N < k + 3, 2 = one value only.  summary: the cases (binary) or
// the mean (quant).  cols[A][16] and chol[k1][k1] are what the backend reads (filled when fit is 1).
struct GlmNull {
	int32_t N = 0, iter = 0, fit = 0, skip = 0;
	double summary = 0;
	std::vector<double> cols, chol;
};

// Z'WZ of the rows z[N][k1] with the weights w[N] (nullptr: 1)
void glm_gram(const std::vector<double> &z, const double *w, int32_t N, int32_t k1, std::vector<double> &H)
{
	H.assign((size_t)(k1 * k1), 0.0);
	for (int32_t i = 0; i < N; ++i) {
		const double *zi = z.data() + (size_t)i * (size_t)k1;
		const double wi = w ? w[i] : 1.0;
		for (int32_t a = 0; a < k1; ++a)
			for (int32_t b = 0; b <= a; ++b) H[(size_t)(a * k1 + b)] += wi * zi[a] * zi[b];
	}
	for (int32_t a = 0; a < k1; ++a)
		for (int32_t b = a + 1; b < k1; ++b) H[(size_t)(a * k1 + b)] = H[(size_t)(b * k1 + a)];
}

// the null model of one trait: val[A] (NaN = missing) on the intercept and cov[A][k]
void glm_null(const double *val, const double *cov, int32_t A, int32_t k, int32_t family, GlmNull &r)
{
	r = GlmNull();
	const int32_t k1 = k + 1;
	std::vector<int32_t> col;
	for (int32_t c = 0; c < A; ++c) if (val[c] == val[c]) col.push_back(c);
	const int32_t N = r.N = (int32_t)col.size();
	double sum = 0;
	bool flat = true;
	for (int32_t i = 0; i < N; ++i) sum += val[col[(size_t)i]], flat = flat && val[col[(size_t)i]] == val[col[0]];
	r.summary = family == PG_GLM_BINARY ? sum : N ? sum / (double)N : 0.0;
	if (N < k + 3) { r.skip = 1; return; }
	if (flat) { r.skip = 2; return; }
	std::vector<double> z((size_t)N * (size_t)k1), y((size_t)N), eta((size_t)N), mu((size_t)N), w((size_t)N), res((size_t)N), H, g((size_t)k1), beta((size_t)k1, 0.0);
	for (int32_t i = 0; i < N; ++i) {
		y[(size_t)i] = val[col[(size_t)i]];
		z[(size_t)i * (size_t)k1] = 1.0;
		for (int32_t j = 0; j < k; ++j) z[(size_t)i * (size_t)k1 + 1 + (size_t)j] = cov[(size_t)col[(size_t)i] * (size_t)k + (size_t)j];
	}
	auto linear = [&](const std::vector<double> &b) {
		for (int32_t i = 0; i < N; ++i) {
			double e = 0;
			for (int32_t j = 0; j < k1; ++j) e += z[(size_t)i * (size_t)k1 + (size_t)j] * b[(size_t)j];
			eta[(size_t)i] = e;
		}
	};
	auto gradient = [&]() { // Z'(y - mu)
		std::fill(g.begin(), g.end(), 0.0);
		for (int32_t i = 0; i < N; ++i)
			for (int32_t j = 0; j < k1; ++j) g[(size_t)j] += z[(size_t)i * (size_t)k1 + (size_t)j] * (y[(size_t)i] - mu[(size_t)i]);
	};
	if (family == PG_GLM_BINARY) {
		auto loglik = [&](const std::vector<double> &b) { // the sum of y eta - log(1 + e^eta)
			linear(b);
			double ll = 0;
			for (int32_t i = 0; i < N; ++i) ll += y[(size_t)i] * eta[(size_t)i] - (std::max(eta[(size_t)i], 0.0) + std::log1p(std::exp(-std::fabs(eta[(size_t)i]))));
			return ll;
		};
		auto moments = [&]() { // from eta
			for (int32_t i = 0; i < N; ++i) mu[(size_t)i] = 1.0 / (1.0 + std::exp(-eta[(size_t)i])), w[(size_t)i] = mu[(size_t)i] * (1.0 - mu[(size_t)i]);
		};
		const double ybar = sum / (double)N;
		beta[0] = std::log(ybar / (1.0 - ybar));
		double ll = loglik(beta);
		bool converged = false;
		std::vector<double> cand((size_t)k1);
		for (int32_t it = 1; it <= GLM_MAX_ITER && !converged; ++it) {
			linear(beta), moments(), gradient();
			glm_gram(z, w.data(), N, k1, H);
			if (!glm_chol(H, k1)) return; // fit 0
			glm_solve(H, k1, g);          // the Newton step
			double llc = ll;
			for (int32_t h = 0;; ++h) {
				for (int32_t j = 0; j < k1; ++j) cand[(size_t)j] = beta[(size_t)j] + g[(size_t)j];
				llc = loglik(cand);
				if (llc >= ll - GLM_LL_NOISE * (1.0 + std::fabs(ll)) || h == GLM_MAX_HALVE) break; // (a fall within the rounding of the sum is none: near the optimum the full step stands)
				for (int32_t j = 0; j < k1; ++j) g[(size_t)j] *= 0.5;
			}
			beta = cand, ll = llc, r.iter = it;
			double step = 0;
			for (int32_t j = 0; j < k1; ++j) step = std::max(step, std::fabs(g[(size_t)j]));
			converged = step <= GLM_STEP;
		}
		if (!converged) return;
		linear(beta);
		for (int32_t i = 0; i < N; ++i) if (!(std::fabs(eta[(size_t)i]) <= GLM_ETA)) return; // separation
		moments();
		for (int32_t i = 0; i < N; ++i) res[(size_t)i] = y[(size_t)i] - mu[(size_t)i];
		glm_gram(z, w.data(), N, k1, H);
		if (!glm_chol(H, k1)) return;
	} else {
		glm_gram(z, nullptr, N, k1, H);
		if (!glm_chol(H, k1)) return;
		std::fill(mu.begin(), mu.end(), 0.0);
		gradient(); // Z'y
		glm_solve(H, k1, g);
		linear(g);
		double rss = 0;
		for (int32_t i = 0; i < N; ++i) rss += (y[(size_t)i] - eta[(size_t)i]) * (y[(size_t)i] - eta[(size_t)i]);
		const double s2 = rss / (double)(N - k1);
		if (!(s2 > 0) || !std::isfinite(1.0 / s2)) return; // an exact fit: no residual variance to test against
		for (int32_t i = 0; i < N; ++i) res[(size_t)i] = (y[(size_t)i] - eta[(size_t)i]) / s2, w[(size_t)i] = 1.0 / s2;
		const double s = std::sqrt(s2);
		for (double &x : H) x /= s; // the factor of Z'WZ = Z'Z / s2
	}
	r.fit = 1, r.chol = H;
	r.cols.assign((size_t)A * GLM_COLS, 0.0);
	for (int32_t i = 0; i < N; ++i) {
		double *c = r.cols.data() + (size_t)col[(size_t)i] * GLM_COLS;
		c[0] = 1.0, c[1] = res[(size_t)i], c[2] = w[(size_t)i];
		for (int32_t j = 0; j < k; ++j) c[3 + j] = w[(size_t)i] * z[(size_t)i * (size_t)k1 + 1 + (size_t)j];
	}
}

// The second implementation of the backend's step: the sums of every (trait, gene) by walking the set bits in fp64, in ascending order of
// the assembly, then the same forward substitution.  bits[G][W], cols[T][A][16], chol[T][k1][k1]; a, u, v, sw[T][G]
void glm_host(const uint32_t *bits, const double *cols, const double *chol, int32_t G, int32_t A, int32_t T, int32_t k1, std::vector<int32_t> &a, std::vector<double> &u,
              std::vector<double> &v, std::vector<double> &sw)
{
	const int32_t W = (A + 31) / 32;
	for (int32_t t = 0; t < T; ++t) {
		const double *ct = cols + (size_t)t * (size_t)A * GLM_COLS, *L = chol + (size_t)t * (size_t)(k1 * k1);
		for (int32_t g = 0; g < G; ++g) {
			double S[GLM_COLS] = {0}, y[GLM_MAX_COV + 1], q = 0;
			const uint32_t *b = bits + (size_t)g * (size_t)W;
			for (int32_t w = 0; w < W; ++w)
				for (uint32_t x = b[w]; x; x &= x - 1) {
					const double *c = ct + (size_t)(w * 32 + __builtin_ctz(x)) * GLM_COLS;
					for (int32_t j = 0; j < k1 + 2; ++j) S[j] += c[j];
				}
			for (int32_t i = 0; i < k1; ++i) {
				double s = S[2 + i];
				for (int32_t j = 0; j < i; ++j) s -= L[i * k1 + j] * y[j];
				y[i] = s / L[i * k1 + i];
				q += y[i] * y[i];
			}
			const size_t at = (size_t)t * (size_t)G + (size_t)g;
			a[at] = (int32_t)S[0], u[at] = S[1], sw[at] = S[2], v[at] = S[2] - q;
		}
	}
}

double t_glm = 0; // seconds of the backend step (or the second implementation) of the last command

// Every trait of val[T][A] (NaN = missing) over bits[G][W] (gene-major, the bits past A zero) with the covariates cov[A][k]: the null fits,
// then a, u, v, sw[T][G] of the fitted traits in one backend call (the rows of the others stay zero).  0 or a PGA_ERR_* code
struct Glm { std::vector<GlmNull> null; std::vector<int32_t> a; std::vector<double> u, v, sw; };

int glm_core(const std::vector<uint32_t> &bits, int32_t G, int32_t A, const double *val, int32_t T, const double *cov, int32_t k, int32_t family, Glm &r)
{
	if (A > GLM_MAX_COL || k > GLM_MAX_COV) return PGA_ERR_RANGE;
	const int32_t k1 = k + 1;
	const size_t tg = (size_t)T * (size_t)G;
	r.null.assign((size_t)T, GlmNull());
	r.a.assign(tg, 0), r.u.assign(tg, 0.0), r.v.assign(tg, 0.0), r.sw.assign(tg, 0.0);
	std::vector<int32_t> fitted;
	std::vector<double> cols, chol;
	for (int32_t t = 0; t < T; ++t) {
		GlmNull &n = r.null[(size_t)t];
		glm_null(val + (size_t)t * (size_t)A, cov, A, k, family, n);
		if (!n.fit) continue;
		fitted.push_back(t);
		cols.insert(cols.end(), n.cols.begin(), n.cols.end()), chol.insert(chol.end(), n.chol.begin(), n.chol.end());
		std::vector<double>().swap(n.cols);
	}
	const int32_t Tf = (int32_t)fitted.size();
	if (Tf == 0 || G == 0) return 0;
	const size_t fg = (size_t)Tf * (size_t)G;
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	int rc = 0;
	std::vector<int32_t> a(fg);
	std::vector<double> u(fg), v(fg), sw(fg);
	if (be->pan_glm != nullptr) {
		const pga_glm_in_t in{bits.data(), cols.data(), chol.data(), G, A, Tf, k, nullptr};
		pga_glm_out_t res{};
		if ((rc = be->pan_glm(&in, &res)) == 0) a.assign(res.a, res.a + fg), u.assign(res.u, res.u + fg), v.assign(res.v, res.v + fg), sw.assign(res.sw, res.sw + fg);
	} else glm_host(bits.data(), cols.data(), chol.data(), G, A, Tf, k1, a, u, v, sw);
	t_glm += now_sec() - t0;
	if (rc != 0) return rc;
	for (int32_t f = 0; f < Tf; ++f) {
		const size_t from = (size_t)f * (size_t)G, to = (size_t)fitted[(size_t)f] * (size_t)G;
		std::copy(a.begin() + from, a.begin() + from + G, r.a.begin() + to), std::copy(u.begin() + from, u.begin() + from + G, r.u.begin() + to);
		std::copy(v.begin() + from, v.begin() + from + G, r.v.begin() + to), std::copy(sw.begin() + from, sw.begin() + from + G, r.sw.begin() + to);
	}
	return 0;
}

inline bool glm_eligible(int32_t a, int32_t N, int32_t min_count) { return std::min(a, N - a) >= min_count; }
inline bool glm_collinear(double v, double sw) { return !(v > GLM_COLLINEAR * sw); }

bool glm_opt_ok(const pg_glm_opt_t *o)
{
	return o != nullptr && (o->type == PG_DIST_GENE || o->type == PG_DIST_ADJ) && (o->metric == PG_DIST_JACCARD || o->metric == PG_DIST_DIFF) &&
	       (o->family == PG_GLM_BINARY || o->family == PG_GLM_QUANT) && o->min_count >= 1 && o->max_p == o->max_p;
}

// assembly-major item rows [A][(M + 31) / 32] -> item-major rows [M][(A + 31) / 32]
void glm_transpose(const std::vector<uint32_t> &in, int32_t M, int32_t A, std::vector<uint32_t> &out)
{
	const size_t Wi = ((size_t)M + 31) / 32, Wo = ((size_t)A + 31) / 32;
	out.assign((size_t)M * Wo, 0);
	for (int32_t x = 0; x < A; ++x) {
		const uint32_t *row = in.data() + (size_t)x * Wi;
		for (size_t w = 0; w < Wi; ++w)
			for (uint32_t b = row[w]; b; b &= b - 1) out[(w * 32 + (size_t)__builtin_ctz(b)) * Wo + (size_t)(x >> 5)] |= 1u << (x & 31);
	}
}

// the genes, the trait file, the axes of the distance, the null fits and the score statistics, then the text
int glm_run(const ItemSource &src, const char *trait_fn, const pg_glm_opt_t *o)
{
	const double t_start = now_sec();
	if (o->type != PG_DIST_GENE && o->type != PG_DIST_ADJ) return PGA_ERR_ARG;
	std::vector<std::string> names, gene;
	std::vector<uint32_t> gbits, dbits;
	int32_t G, M;
	if (src(PG_DIST_GENE, names, gbits, G, &gene) != 0) return PAN_NO_ITEMS;
	const int32_t A = (int32_t)names.size();
	const bool binary = o->family == PG_GLM_BINARY;
	std::vector<std::string> trait;
	std::vector<double> val;
	if (binary || o->family != PG_GLM_QUANT) {
		Traits tr;
		if (read_traits(trait_fn, names, tr) != 0) return PAN_BAD_FILE;
		trait = tr.name, val.resize(tr.lab.size());
		for (size_t i = 0; i < val.size(); ++i) val[i] = tr.lab[i] < 0 ? std::nan("") : (double)tr.lab[i];
	} else {
		QTraits tr;
		if (read_qtraits(trait_fn, names, tr) != 0) return PAN_BAD_FILE;
		trait = tr.name, val = tr.val;
	}
	if (!glm_opt_ok(o)) return PGA_ERR_ARG;
	if (o->n_axis < 0 || o->n_axis > GLM_MAX_COV || A > GLM_MAX_COL) return PGA_ERR_RANGE;
	if (o->type == PG_DIST_ADJ) {
		std::vector<std::string> again;
		if (src(PG_DIST_ADJ, again, dbits, M) != 0) return PAN_NO_ITEMS;
	}
	const double t_prep = now_sec() - t_start;
	// the covariates: the principal coordinates of all assemblies, every axis at unit variance
	int32_t F = 20, k = 0, converged = 1;
	std::vector<double> cov;
	double t_axes = 0;
	if (o->n_axis > 0) {
		const double t0 = now_sec();
		std::vector<int32_t> q;
		if (const int rc = fixed_dist(o->type == PG_DIST_ADJ ? dbits : gbits, o->type == PG_DIST_ADJ ? M : G, A, o->metric, q, &F)) return rc;
		Pcoa pc;
		if (const int rc = pcoa_core(q.data(), A, F, o->n_axis, o->seed, pc)) return rc;
		k = pc.n_axis, converged = pc.skip ? 1 : pc.converged;
		cov.resize((size_t)A * (size_t)k);
		for (int32_t a = 0; a < k; ++a) {
			const double sd = std::sqrt(pc.eig[(size_t)a] / (double)A);
			for (size_t x = 0; x < (size_t)A; ++x) cov[x * (size_t)k + (size_t)a] = pc.coord[x * (size_t)k + (size_t)a] / sd;
		}
		t_axes = now_sec() - t0;
		if (!converged) std::fprintf(stderr, "Note: pangene glm: the axes did not converge; see pangene pcoa\n");
	}
	std::vector<uint32_t> bits;
	glm_transpose(gbits, G, A, bits);
	t_glm = 0;
	const int32_t T = (int32_t)trait.size();
	Glm r;
	if (const int rc = glm_core(bits, G, A, val.data(), T, cov.data(), k, o->family, r)) return rc;
	OutBuf ob;
	std::string &s = ob.s, lines;
	char b[320];
	std::snprintf(b, sizeof(b), "#\titems %s\tmetric %s\tA %d\tFbits %d\taxes %d\tfamily %s\tconverged %d\n", o->type == PG_DIST_GENE ? "gene" : "adj",
	              o->metric == PG_DIST_JACCARD ? "jaccard" : "diff", A, F, k, binary ? "binary" : "quant", converged);
	s = b;
	s += binary ? "T\tTrait\tN\tCases\tIter\tFit\tTested\tCollinear\tLambda\n" : "T\tTrait\tN\tMean\tIter\tFit\tTested\tCollinear\tLambda\n";
	for (int32_t t = 0; t < T; ++t) {
		const GlmNull &n = r.null[(size_t)t];
		const char *name = trait[(size_t)t].c_str();
		if (n.skip) {
			std::fprintf(stderr, "Note: trait %s has %s over its %d assemblies; skipped\n", name, n.skip == 2 ? "one value" : "too few values for the covariates", n.N);
			continue;
		}
		if (!n.fit) std::fprintf(stderr, "Note: trait %s: the null model did not converge or is separated by the covariates (%d iterations); no genes tested\n", name, n.iter);
		const size_t at = (size_t)t * (size_t)G;
		std::vector<int32_t> el, tested;
		std::vector<double> z, p, q;
		for (int32_t g = 0; n.fit && g < G; ++g) {
			if (!glm_eligible(r.a[at + (size_t)g], n.N, o->min_count)) continue;
			el.push_back(g);
			if (glm_collinear(r.v[at + (size_t)g], r.sw[at + (size_t)g])) continue;
			tested.push_back(g);
			z.push_back(r.u[at + (size_t)g] / std::sqrt(r.v[at + (size_t)g]));
			p.push_back(std::erfc(std::fabs(z.back()) / std::sqrt(2.0)));
		}
		bh_q(p, q);
		std::snprintf(b, sizeof(b), "T\t%s\t%d\t%.6g\t%d\t%d\t%zu\t%zu\t", name, n.N, n.summary, n.iter, n.fit, tested.size(), el.size() - tested.size());
		s += b;
		if (tested.empty()) s += "NA\n";
		else {
			std::vector<double> z2(z.size());
			for (size_t i = 0; i < z.size(); ++i) z2[i] = z[i] * z[i];
			std::sort(z2.begin(), z2.end());
			const size_t m = z2.size();
			std::snprintf(b, sizeof(b), "%.6g\n", (m & 1 ? z2[m / 2] : 0.5 * (z2[m / 2 - 1] + z2[m / 2])) / GLM_CHI2_MEDIAN);
			s += b;
		}
		size_t e = 0;
		for (const int32_t g : el) {
			const double U = r.u[at + (size_t)g], V = r.v[at + (size_t)g];
			const bool is_tested = e < tested.size() && tested[e] == g;
			if (is_tested && !(p[e] <= o->max_p)) { ++e; continue; }
			lines += "G\t", lines += name, lines += '\t', lines += gene[(size_t)g];
			if (is_tested) std::snprintf(b, sizeof(b), "\t%d\t%d\t%.6g\t%.6g\t%.6g\t%.6g\t%.6g\n", n.N, r.a[at + (size_t)g], U / V, 1.0 / std::sqrt(V), z[e], p[e], q[e]), ++e;
			else std::snprintf(b, sizeof(b), "\t%d\t%d\tNA\tNA\tNA\tNA\tNA\n", n.N, r.a[at + (size_t)g]); // collinear with the covariates
			lines += b;
		}
	}
	s += "G\tTrait\tGene\tN\ta\tBeta\tSE\tZ\tp\tq\n";
	s += lines;
	ob.finish();
	if (std::getenv("PANGENE_GLM_TIMING") != nullptr)
		std::fprintf(stderr, "[glm-timing] route=%s genes=%d assemblies=%d traits=%d axes=%d prep_ms=%.3f axes_ms=%.3f stat_ms=%.3f all_ms=%.3f\n", src.route(), G, A, T, k,
		             t_prep * 1e3, t_axes * 1e3, t_glm * 1e3, (now_sec() - t_start) * 1e3);
	return 0;
}

} // namespace
} // namespace pgx

extern "C" {

void pg_glm_opt_init(pg_glm_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->family = PG_GLM_BINARY, o->n_axis = 3, o->seed = 0, o->min_count = 1, o->max_p = 1.0;
}

int pg_glm_file(const char *gfa_fn, const char *trait_fn, const pg_glm_opt_t *o)
{
	if (o == nullptr) { std::fprintf(stderr, "Error: pangene glm: no options\n"); return -2; }
	return file_result(glm_run(items_of_file(gfa_fn), trait_fn, o), gfa_fn, "pangene glm");
}

void pg_write_glm(pg_graph_t *q, const char *trait_fn, const pg_glm_opt_t *o)
{
	if (o == nullptr) { set_error(PGA_ERR_ARG, "pg_write_glm"); return; }
	graph_result(glm_run(items_of_graph(q), trait_fn, o), "pg_write_glm", "pg_write_glm: bad trait file");
}

int pg_pan_glm(const uint8_t *presence, const double *values, int32_t n_gene, int32_t n_asm, int32_t n_trait, const double *covariates, int32_t n_cov, int32_t family,
               const pg_glm_opt_t *o, double *out, int32_t *info)
{
	if (n_gene < 0 || n_asm < 0 || n_trait < 0 || n_cov < 0 || o == nullptr || o->min_count < 1 || (family != PG_GLM_BINARY && family != PG_GLM_QUANT)) return PGA_ERR_ARG;
	if (n_cov > GLM_MAX_COV || n_asm > GLM_MAX_COL) return PGA_ERR_RANGE; // (before the arrays are looked at)
	if (((size_t)n_gene * (size_t)n_asm > 0 && presence == nullptr) || ((size_t)n_trait * (size_t)n_asm > 0 && values == nullptr)) return PGA_ERR_ARG;
	if (((size_t)n_cov * (size_t)n_asm > 0 && covariates == nullptr) || ((size_t)n_trait * (size_t)n_gene > 0 && out == nullptr) || (n_trait > 0 && info == nullptr)) return PGA_ERR_ARG;
	for (size_t i = 0; i < (size_t)n_trait * (size_t)n_asm; ++i) {
		const double v = values[i];
		if (v != v) continue;
		if (!std::isfinite(v) || (family == PG_GLM_BINARY && v != 0.0 && v != 1.0)) return PGA_ERR_ARG;
	}
	for (size_t i = 0; i < (size_t)n_cov * (size_t)n_asm; ++i) if (!std::isfinite(covariates[i])) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_rows(presence, n_gene, n_asm, bits);
	Glm r;
	t_glm = 0;
	if (const int rc = glm_core(bits, n_gene, n_asm, values, n_trait, covariates, n_cov, family, r)) return rc;
	if (std::getenv("PANGENE_GLM_TIMING") != nullptr)
		std::fprintf(stderr, "[glm-timing] route=array genes=%d assemblies=%d traits=%d axes=%d stat_ms=%.3f\n", n_gene, n_asm, n_trait, n_cov, t_glm * 1e3);
	for (int32_t t = 0; t < n_trait; ++t) {
		const GlmNull &n = r.null[(size_t)t];
		int32_t tested = 0;
		for (int32_t g = 0; g < n_gene; ++g) {
			const size_t at = (size_t)t * (size_t)n_gene + (size_t)g;
			const bool e = n.fit && glm_eligible(r.a[at], n.N, o->min_count);
			double *p = out + 4 * at;
			p[0] = e ? (double)r.a[at] : -1.0, p[1] = e ? r.u[at] : 0.0, p[2] = e ? r.v[at] : 0.0, p[3] = e ? r.sw[at] : 0.0;
			tested += e && !glm_collinear(r.v[at], r.sw[at]);
		}
		int32_t *w = info + 4 * (size_t)t;
		w[0] = n.N, w[1] = n.iter, w[2] = n.fit, w[3] = tested;
	}
	return 0;
}

} // extern "C"
