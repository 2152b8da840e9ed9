// pan_pcoa.hpp -- principal coordinates of the assemblies (pg_pcoa_file, pg_write_pcoa, pg_pan_pcoa, pg_pan_pcoa_presence, pangene pcoa;
// DESIGN.md section 8 "Principal coordinates"): classical scaling of the fixed-point distances of pan_tree.hpp.  The option checks, the
// exact trace, the sign rule, the scaling to coordinates and the text are code both builds share; the largest eigenpairs of the
// Gower-centred matrix come from the backend (pga_pan_pcoa: Lanczos on the device) or, when the backend has no such entry, from the
// second implementation below: cyclic Jacobi on the dense matrix, an independent algorithm that exists for the tests.
// This is the project's floating-point command: two builds agree within the tolerances DESIGN.md derives from the stopping rule, not
// byte for byte.

namespace pgx {
namespace {

constexpr int32_t PCOA_MAX_COL = 16384, PCOA_MAX_AXIS = 16, PCOA_MAX_STEP = 256; // the backend's limits (include/pangene_hip.h pga_pan_pcoa)
constexpr int32_t PCOA_JACOBI_MAX = 2048;                                        // the second implementation's
constexpr double PCOA_KEEP = 1e-9;                                               // axis a is reported when lambda_a > PCOA_KEEP lambda_1

// what one matrix leaves.  skip: 0 = done, 1 = N < 3, 2 = every distance is zero.  eig, resid[n_axis]; vec[N][n_axis] unit columns as
// the solver left them; coord[N][n_axis] after the sign rule and the scaling
struct Pcoa {
	int32_t N = 0, n_axis = 0, steps = 0, restarts = 0, converged = 0, skip = 1;
	double trace = 0;
	std::vector<double> eig, resid, coord;
};

// The second implementation: B = J A J formed densely, then cyclic Jacobi rotations until no off-diagonal entry is left above
// 2^-53 |B|_F / N.  k pairs, the largest first; the residuals are computed from a copy of B.  `steps` counts the sweeps.
int pcoa_jacobi(const int32_t *q, int32_t N, int32_t F, int32_t k, Pcoa &r, std::vector<double> &vec)
{
	if (N > PCOA_JACOBI_MAX) return PGA_ERR_RANGE;
	const size_t n = (size_t)N;
	std::vector<double> B(n * n), rm(n, 0.0), V(n * n, 0.0);
	const double scale = -std::ldexp(1.0, -2 * F - 1);
	double gm = 0;
	for (size_t i = 0; i < n; ++i) {
		for (size_t j = 0; j < n; ++j) { const double d = (double)q[i * n + j]; B[i * n + j] = scale * (d * d), rm[i] += B[i * n + j]; }
		rm[i] /= (double)N, gm += rm[i];
	}
	gm /= (double)N;
	double fro = 0;
	for (size_t i = 0; i < n; ++i)
		for (size_t j = 0; j < n; ++j) { B[i * n + j] += gm - rm[i] - rm[j]; fro += B[i * n + j] * B[i * n + j]; }
	for (size_t i = 0; i < n; ++i)
		for (size_t j = i + 1; j < n; ++j) B[i * n + j] = B[j * n + i] = 0.5 * (B[i * n + j] + B[j * n + i]);
	const std::vector<double> B0 = B;
	for (size_t i = 0; i < n; ++i) V[i * n + i] = 1.0;
	const double small = std::ldexp(std::sqrt(fro), -53) / (double)N;
	r.steps = 0;
	for (bool turned = true; turned && r.steps < 100; ++r.steps) {
		turned = false;
		for (size_t p = 0; p + 1 < n; ++p)
			for (size_t s = p + 1; s < n; ++s) {
				const double bps = B[p * n + s];
				if (std::fabs(bps) <= small) continue;
				turned = true;
				const double theta = (B[s * n + s] - B[p * n + p]) / (2.0 * bps);
				const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
				const double c = 1.0 / std::sqrt(t * t + 1.0), sn = t * c;
				for (size_t i = 0; i < n; ++i) { // columns p and s
					const double x = B[i * n + p], y = B[i * n + s];
					B[i * n + p] = c * x - sn * y, B[i * n + s] = sn * x + c * y;
				}
				for (size_t i = 0; i < n; ++i) { // rows p and s
					const double x = B[p * n + i], y = B[s * n + i];
					B[p * n + i] = c * x - sn * y, B[s * n + i] = sn * x + c * y;
				}
				B[p * n + s] = B[s * n + p] = 0.0;
				for (size_t i = 0; i < n; ++i) {
					const double x = V[i * n + p], y = V[i * n + s];
					V[i * n + p] = c * x - sn * y, V[i * n + s] = sn * x + c * y;
				}
			}
	}
	// The centring leaves the constant vector with the eigenvalue 0; it is no axis.  It is the column closest to 1 / sqrt(N).
	size_t ones = 0;
	double best = -1;
	for (size_t c = 0; c < n; ++c) {
		double s = 0;
		for (size_t i = 0; i < n; ++i) s += V[i * n + c];
		if (std::fabs(s) > best) best = std::fabs(s), ones = c;
	}
	std::vector<size_t> idx;
	for (size_t c = 0; c < n; ++c) if (c != ones) idx.push_back(c);
	std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return B[a * n + a] > B[b * n + b]; });
	const size_t ka = std::min(idx.size(), (size_t)k);
	r.eig.assign(ka, 0.0), r.resid.assign(ka, 0.0), vec.assign(n * ka, 0.0);
	for (size_t a = 0; a < ka; ++a) {
		const size_t c = idx[a];
		r.eig[a] = B[c * n + c];
		double res = 0;
		for (size_t i = 0; i < n; ++i) {
			double s = 0;
			for (size_t j = 0; j < n; ++j) s += B0[i * n + j] * V[j * n + c];
			s -= r.eig[a] * V[i * n + c], res += s * s;
			vec[i * ka + a] = V[i * n + c];
		}
		r.resid[a] = std::sqrt(res);
	}
	r.n_axis = (int32_t)ka, r.restarts = 0, r.converged = 1;
	return 0;
}

double t_pcoa = 0; // seconds of the backend step (or the second implementation) of the last command

// the vectors the iteration may use: 256, or PANGENE_PCOA_STEPS (tests)
int32_t pcoa_max_step()
{
	if (const char *s = std::getenv("PANGENE_PCOA_STEPS")) { const long v = std::atol(s); if (v >= 1 && v <= PCOA_MAX_STEP) return (int32_t)v; }
	return PCOA_MAX_STEP;
}

// q[N][N], checked (symmetric, zero diagonal, entries in [0, 2^29)), with F fraction bits: the k largest pairs, the exact trace, the
// coordinates; 0 or a PGA_ERR_* code
int pcoa_core(const int32_t *q, int32_t N, int32_t F, int32_t k, uint32_t seed, Pcoa &r)
{
	r = Pcoa();
	r.N = N;
	if (N > PCOA_MAX_COL || k < 1 || k > PCOA_MAX_AXIS) return PGA_ERR_RANGE;
	if (F < 0 || F > 30) return PGA_ERR_ARG;
	const size_t n = (size_t)N;
	unsigned __int128 T = 0; // the sum of q^2 over i != j (the diagonal is zero): below 2^58 2^28
	for (size_t i = 0; i < n * n; ++i) T += (unsigned __int128)((uint64_t)q[i] * (uint64_t)q[i]);
	if (N < 3) return 0;
	if (T == 0) { r.skip = 2; return 0; }
	r.skip = 0;
	r.trace = ratio((i128)T, 2 * (i128)N, 2 * F); // trace(B) = T / (2 N) 4^-F: the sum of ALL eigenvalues, the negative ones included
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	std::vector<double> own;
	const double *vec = nullptr;
	int rc = 0;
	if (be->pan_pcoa != nullptr) {
		const pga_pcoa_in_t in{q, N, F, k, seed, pcoa_max_step(), nullptr, nullptr, 0};
		pga_pcoa_out_t res{};
		if ((rc = be->pan_pcoa(&in, &res)) == 0) {
			r.n_axis = res.n_axis, r.steps = res.n_step, r.restarts = res.n_restart, r.converged = res.converged;
			r.eig.assign(res.eig, res.eig + res.n_axis), r.resid.assign(res.resid, res.resid + res.n_axis);
			vec = res.vec;
		}
	} else if ((rc = pcoa_jacobi(q, N, F, std::min(k, N - 1), r, own)) == 0) vec = own.data();
	t_pcoa += now_sec() - t0;
	if (rc != 0) return rc;
	// the axes above PCOA_KEEP lambda_1; the sign rule (the component largest in size is positive, the first one on a tie); x = v sqrt(lambda)
	const int32_t have = r.n_axis;
	int32_t keep = 0;
	while (keep < have && r.eig[0] > 0 && r.eig[(size_t)keep] > PCOA_KEEP * r.eig[0]) ++keep;
	r.coord.assign(n * (size_t)keep, 0.0);
	for (int32_t a = 0; a < keep; ++a) {
		size_t at = 0;
		for (size_t i = 1; i < n; ++i) if (std::fabs(vec[i * (size_t)have + a]) > std::fabs(vec[at * (size_t)have + a])) at = i;
		const double f = (vec[at * (size_t)have + a] < 0 ? -1.0 : 1.0) * std::sqrt(r.eig[(size_t)a]);
		for (size_t i = 0; i < n; ++i) r.coord[i * (size_t)keep + a] = f * vec[i * (size_t)have + a];
	}
	r.n_axis = keep, r.eig.resize((size_t)keep), r.resid.resize((size_t)keep);
	return 0;
}

bool pcoa_opt_ok(const pg_pcoa_opt_t *o)
{
	return o != nullptr && (o->type == PG_DIST_GENE || o->type == PG_DIST_ADJ) && (o->metric == PG_DIST_JACCARD || o->metric == PG_DIST_DIFF);
}

// the items, the distances, the axes, then the text
int pcoa_run(const ItemSource &src, const pg_pcoa_opt_t *o)
{
	const double t_start = now_sec();
	std::vector<std::string> names;
	std::vector<uint32_t> bits;
	int32_t M;
	if (src(o->type, names, bits, M) != 0) return PAN_NO_ITEMS;
	if (!pcoa_opt_ok(o)) return PGA_ERR_ARG;
	if (o->n_axis < 1 || o->n_axis > PCOA_MAX_AXIS) return PGA_ERR_RANGE;
	const int32_t A = (int32_t)names.size();
	const double t_prep = now_sec() - t_start;
	std::vector<int32_t> q;
	int32_t F = 20;
	if (const int rc = fixed_dist(bits, M, A, o->metric, q, &F)) return rc;
	t_pcoa = 0;
	Pcoa r;
	if (const int rc = pcoa_core(q.data(), A, F, o->n_axis, o->seed, r)) return rc;
	OutBuf ob;
	std::string &s = ob.s;
	char b[256];
	std::snprintf(b, sizeof(b), "#\titems %s\tmetric %s\tN %d\tFbits %d\ttrace %.6g\tsteps %d\trestarts %d\tconverged %d\n", o->type == PG_DIST_GENE ? "gene" : "adj",
	              o->metric == PG_DIST_JACCARD ? "jaccard" : "diff", A, F, r.trace, r.steps, r.restarts, r.skip ? 1 : r.converged);
	s = b;
	if (r.skip) std::fprintf(stderr, "Note: %s over the %d assemblies; no principal coordinates\n", r.skip == 2 ? "no distance above zero" : "fewer than 3 assemblies", A);
	else {
		if (!r.converged)
			std::fprintf(stderr, "Note: pangene pcoa: the axes did not converge within %d vectors; their residuals are in the table\n", r.steps);
		s += "EV\tAxis\tEigenvalue\tExplained\tCumulative\tResidual\n";
		double cum = 0;
		for (int32_t a = 0; a < r.n_axis; ++a) {
			const double part = r.eig[(size_t)a] / r.trace;
			cum += part;
			std::snprintf(b, sizeof(b), "EV\t%d\t%.6g\t%.4f\t%.4f\t%.6g\n", a + 1, r.eig[(size_t)a], part, cum, r.resid[(size_t)a]);
			s += b;
		}
		s += "PC\tAsm";
		for (int32_t a = 0; a < r.n_axis; ++a) s += "\tPC" + std::to_string(a + 1);
		s += '\n';
		for (size_t x = 0; x < (size_t)A; ++x) {
			s += "PC\t" + names[x];
			for (int32_t a = 0; a < r.n_axis; ++a) { std::snprintf(b, sizeof(b), "\t%.6g", r.coord[x * (size_t)r.n_axis + (size_t)a]); s += b; }
			s += '\n';
			ob.flush_if_full();
		}
	}
	ob.finish();
	if (std::getenv("PANGENE_PCOA_TIMING") != nullptr)
		std::fprintf(stderr, "[pcoa-timing] route=%s items=%d assemblies=%d axes=%d steps=%d restarts=%d converged=%d prep_ms=%.3f eig_ms=%.3f all_ms=%.3f\n", src.route(), M, A,
		             r.n_axis, r.steps, r.restarts, r.converged, t_prep * 1e3, t_pcoa * 1e3, (now_sec() - t_start) * 1e3);
	return 0;
}

// a result into the caller's arrays: eig[k], resid[k], coord[n][k] (the columns past the axes are zero), info = axes, steps, converged, restarts
void pcoa_copy(const Pcoa &r, int32_t n, int32_t k, double *eig, double *resid, double *coord, double *trace, int32_t *info)
{
	std::fill(eig, eig + k, 0.0), std::fill(resid, resid + k, 0.0), std::fill(coord, coord + (size_t)n * (size_t)k, 0.0);
	for (int32_t a = 0; a < r.n_axis; ++a) {
		eig[a] = r.eig[(size_t)a], resid[a] = r.resid[(size_t)a];
		for (size_t i = 0; i < (size_t)n; ++i) coord[i * (size_t)k + (size_t)a] = r.coord[i * (size_t)r.n_axis + (size_t)a];
	}
	*trace = r.trace;
	info[0] = r.n_axis, info[1] = r.steps, info[2] = r.skip ? 1 : r.converged, info[3] = r.restarts;
}

} // namespace
} // namespace pgx

extern "C" {

void pg_pcoa_opt_init(pg_pcoa_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->n_axis = 3, o->seed = 0;
}

int pg_pcoa_file(const char *gfa_fn, const pg_pcoa_opt_t *o)
{
	if (o == nullptr) { std::fprintf(stderr, "Error: pangene pcoa: no options\n"); return -2; }
	return file_result(pcoa_run(items_of_file(gfa_fn), o), gfa_fn, "pangene pcoa");
}

void pg_write_pcoa(pg_graph_t *q, const pg_pcoa_opt_t *o)
{
	if (o == nullptr) { set_error(PGA_ERR_ARG, "pg_write_pcoa"); return; }
	graph_result(pcoa_run(items_of_graph(q), o), "pg_write_pcoa");
}

int pg_pan_pcoa(const int32_t *q, int32_t n, int32_t fbits, const pg_pcoa_opt_t *o, double *eig, double *resid, double *coord, double *trace, int32_t *info)
{
	if (n < 0 || o == nullptr || eig == nullptr || resid == nullptr || coord == nullptr || trace == nullptr || info == nullptr || (n > 0 && q == nullptr)) return PGA_ERR_ARG;
	if (n > PCOA_MAX_COL || o->n_axis < 1 || o->n_axis > PCOA_MAX_AXIS) return PGA_ERR_RANGE; // (before the matrix is looked at)
	int rc = fixed_matrix_ok(q, n);
	if (rc != 0) return rc;
	Pcoa r;
	if ((rc = pcoa_core(q, n, fbits, o->n_axis, o->seed, r)) != 0) return rc;
	pcoa_copy(r, n, o->n_axis, eig, resid, coord, trace, info);
	return 0;
}

int pg_pan_pcoa_presence(const uint8_t *presence, int32_t n_item, int32_t n_asm, const pg_pcoa_opt_t *o, double *eig, double *resid, double *coord, double *trace,
                         int32_t *info, int32_t *frac_bits)
{
	if (n_item < 0 || n_asm < 0 || !pcoa_opt_ok(o) || frac_bits == nullptr || ((size_t)n_item * (size_t)n_asm > 0 && presence == nullptr)) return PGA_ERR_ARG;
	if (eig == nullptr || resid == nullptr || coord == nullptr || trace == nullptr || info == nullptr) return PGA_ERR_ARG;
	if (n_asm > PCOA_MAX_COL || o->n_axis < 1 || o->n_axis > PCOA_MAX_AXIS) return PGA_ERR_RANGE;
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	std::vector<int32_t> q;
	*frac_bits = 20;
	if (const int rc = fixed_dist(bits, n_item, n_asm, o->metric, q, frac_bits)) return rc;
	Pcoa r;
	if (const int rc = pcoa_core(q.data(), n_asm, *frac_bits, o->n_axis, o->seed, r)) return rc;
	pcoa_copy(r, n_asm, o->n_axis, eig, resid, coord, trace, info);
	return 0;
}

} // extern "C"
