// pga_pan_pcoa (include/pangene_hip.h): the largest eigenpairs of the Gower-centred matrix of pangene pcoa on the device (k_pcoa.hpp).
// Context-free: it runs on a stream of its own on the current device.  The device buffers and the page-locked results are kept from call
// to call in the PAN_PCOA pool and only ever grow; pga_host_trim(0) gives them back.
//
// The first half of this file is the iteration itself, plain C++ over an `Ops` that makes start vectors, runs chunks of steps and forms
// Ritz vectors (pcoa::lanczos): what is decided between the chunks.  The second half is the Ops of the device and the entry.
//
// The iteration.  Step j takes the unit vector v_j: w = B v_j, two passes of classical Gram-Schmidt against every vector so far (those
// of earlier restarts included), alpha_j = the coefficient on v_j, beta_j = |w|, v_(j+1) = w / beta_j.  Steps are queued PC_CHUNK at a
// time; the host then reads alpha, beta and the flag and solves the tridiagonal eigenproblem (at most 256 x 256, tql2 below).
// beta_j <= 1e-12 |B| is a breakdown: the vectors of the block span an invariant subspace.  The block is locked -- its Ritz pairs are
// eigenpairs, T has a zero where it ends -- and the iteration restarts from a fresh counter-based vector made orthogonal to everything
// locked.  A restart whose first product vanishes has found the remainder null; N - 1 vectors span the whole centred subspace; either
// ends the run.  Otherwise the run ends when the n_axis algebraically largest Ritz pairs all have residuals |beta s| <= 1e-10 theta_1
// and -- after a restart -- the largest Ritz value of the block still running has converged too and is not one of them: the n_axis
// pairs then stand above what is left.  (A Krylov space holds one vector of an eigenspace only; the copies of a multiple eigenvalue are
// found by the restarts, and the last condition keeps the run from stopping while a block may still bring one.)  max_step vectors in
// all end the run as well; `converged` says whether the returned pairs met the residual bound.
#include <cmath>

namespace pcoa {

constexpr int32_t PC_CHUNK = 8;       // steps queued between two reads of alpha, beta and the flag
constexpr double PC_RESID = 1e-10;    // a Ritz pair has converged: residual <= PC_RESID theta_1
constexpr double PC_NULL = 1e-12;     // the breakdown bound, relative to the estimate of |B| (PC_BREAK of k_pcoa.hpp)

// Eigenpairs of the symmetric tridiagonal matrix with diagonal d[n] and off-diagonal e[n] (e[i] couples i and i + 1, e[n - 1] unused) by
// the implicit QL method (tql2 of EISPACK): d becomes the eigenvalues (in no order), z[n][n] row-major: column k is the vector of d[k].
// false after 60 iterations on one eigenvalue
inline bool tql2(int32_t n, std::vector<double> &d, std::vector<double> &e, std::vector<double> &z)
{
	z.assign((size_t)n * (size_t)n, 0.0);
	for (int32_t i = 0; i < n; ++i) z[(size_t)i * n + i] = 1.0;
	if (n == 0) return true;
	e[(size_t)n - 1] = 0.0;
	double f = 0.0, tst1 = 0.0;
	const double eps = 0x1p-52;
	for (int32_t l = 0; l < n; ++l) {
		tst1 = std::max(tst1, std::fabs(d[l]) + std::fabs(e[l]));
		int32_t m = l;
		while (m < n - 1 && std::fabs(e[m]) > eps * tst1) ++m;
		if (m > l) {
			int iter = 0;
			do {
				if (++iter > 60) return false;
				double g = d[l], p = (d[l + 1] - g) / (2.0 * e[l]), r = std::hypot(p, 1.0);
				if (p < 0) r = -r;
				d[l] = e[l] / (p + r), d[l + 1] = e[l] * (p + r);
				const double dl1 = d[l + 1];
				double h = g - d[l];
				for (int32_t i = l + 2; i < n; ++i) d[i] -= h;
				f += h;
				p = d[m];
				double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
				const double el1 = e[l + 1];
				for (int32_t i = m - 1; i >= l; --i) {
					c3 = c2, c2 = c, s2 = s;
					g = c * e[i], h = c * p;
					r = std::hypot(p, e[i]);
					e[i + 1] = s * r, s = e[i] / r, c = p / r;
					p = c * d[i] - s * g;
					d[i + 1] = h + s * (c * g + s * d[i]);
					for (int32_t k = 0; k < n; ++k) {
						double *zk = &z[(size_t)k * n];
						h = zk[i + 1];
						zk[i + 1] = s * zk[i] + c * h, zk[i] = c * zk[i] - s * h;
					}
				}
				p = -s * s2 * c3 * el1 * e[l] / dl1;
				e[l] = s * p, d[l] = c * p;
			} while (std::fabs(e[l]) > eps * tst1);
		}
		d[l] += f, e[l] = 0.0;
	}
	return true;
}

struct Pair { double theta, resid; int32_t lo, hi, col, blk; }; // a Ritz pair: its block [lo, hi), its column of the block's vectors, the block's number
struct Result {
	int32_t n_axis = 0, n_step = 0, n_restart = 0, converged = 0;
	std::vector<double> eig, resid, S; // S[n_axis][n_step]: the pairs' coefficients over the vectors
};

// Ops:  int start(int32_t m, uint32_t restart)            v_m = the start vector of this restart, orthogonal to v_0 .. v_(m-1); 0 or a code
//       int steps(int32_t j0, int32_t nb, double est, double *alpha, double *beta, int32_t *n_done, int32_t *broke)
//                                                          steps j0 .. j0 + nb - 1 as far as they go: alpha[j], beta[j] of those that ran
template <class Ops> int lanczos(Ops &ops, int32_t N, int32_t k, int32_t max_step, Result &out)
{
	out = Result();
	const int32_t dim = N - 1, cap = std::min(max_step, dim); // the centred subspace has N - 1 dimensions
	k = std::min(k, dim);
	if (k < 1) return 0;
	std::vector<double> alpha((size_t)cap + PC_CHUNK, 0.0), beta((size_t)cap + PC_CHUNK, 0.0), d, e;
	std::vector<int32_t> ends;           // where the blocks end: the locked ones, at the end also the one the run stopped in
	std::vector<std::vector<double>> Z;  // the blocks' vectors
	std::vector<Pair> pairs, want;
	auto solve = [&](int32_t blk, int32_t lo, int32_t hi, std::vector<double> &z) { // the pairs of one block, appended to pairs
		const int32_t n = hi - lo;
		d.assign(alpha.begin() + lo, alpha.begin() + hi), e.assign(beta.begin() + lo, beta.begin() + hi);
		if (!tql2(n, d, e, z)) return false;
		for (int32_t c = 0; c < n; ++c) pairs.push_back(Pair{d[(size_t)c], std::fabs(beta[(size_t)hi - 1] * z[(size_t)(n - 1) * n + c]), lo, hi, c, blk});
		return true;
	};
	auto by_theta = [](const Pair &a, const Pair &b) { return a.theta != b.theta ? a.theta > b.theta : a.lo != b.lo ? a.lo < b.lo : a.col < b.col; };
	auto wanted = [&](double &tol) { // the k largest pairs (fewer while there are fewer); true when all of them have converged
		want = pairs;
		std::sort(want.begin(), want.end(), by_theta);
		if ((int32_t)want.size() > k) want.resize((size_t)k);
		tol = want.empty() ? 0.0 : PC_RESID * std::max(want[0].theta, 0.0);
		bool ok = !want.empty();
		for (const Pair &p : want) ok = ok && p.resid <= tol;
		return ok;
	};
	std::vector<Pair> locked; // the pairs of the locked blocks
	std::vector<double> z;
	int32_t m = 0, b0 = 0, restarts = 0; // vectors so far; where the running block starts
	double est = 0.0, tol;
	int rc = ops.start(0, 0);
	if (rc != 0) return rc;
	while (m < cap) {
		const int32_t nb = std::min(PC_CHUNK, cap - m), blk = (int32_t)ends.size();
		int32_t n_done = 0, broke = 0;
		if ((rc = ops.steps(m, nb, est, alpha.data(), beta.data(), &n_done, &broke)) != 0) return rc;
		if (n_done < (broke ? 1 : nb) || n_done > nb) return PGA_ERR_INVARIANT;
		m += n_done;
		pairs = locked;
		if (!solve(blk, b0, m, z)) return PGA_ERR_INVARIANT;
		for (const Pair &p : pairs) est = std::max(est, std::fabs(p.theta));
		if (broke) { // an invariant subspace: lock the block and start again, unless nothing is left
			const bool null_rest = m - b0 == 1 && std::hypot(alpha[(size_t)b0], beta[(size_t)b0]) <= PC_NULL * est;
			ends.push_back(m), locked = pairs, b0 = m;
			if (null_rest || m >= dim || m >= cap) break;
			if ((rc = ops.start(m, (uint32_t)++restarts)) != 0) return rc;
			continue;
		}
		if (!wanted(tol) || (int32_t)want.size() < k) continue;
		if (restarts == 0) break;
		const Pair *top = nullptr; // the largest pair of the running block
		for (const Pair &p : pairs) if (p.blk == blk && (top == nullptr || by_theta(p, *top))) top = &p;
		bool top_wanted = false;
		for (const Pair &p : want) top_wanted = top_wanted || (p.blk == blk && p.col == top->col);
		if (top->resid <= tol && !top_wanted) break;
	}
	if (b0 < m) ends.push_back(m); // the block the run stopped in
	// the pairs as they stand, with their vectors, the largest first
	pairs.clear();
	Z.resize(ends.size());
	for (size_t b = 0; b < ends.size(); ++b)
		if (!solve((int32_t)b, b == 0 ? 0 : ends[b - 1], ends[b], Z[b])) return PGA_ERR_INVARIANT;
	out.converged = wanted(tol) ? 1 : 0;
	out.n_axis = (int32_t)want.size(), out.n_step = m, out.n_restart = restarts;
	out.S.assign((size_t)out.n_axis * (size_t)m, 0.0);
	for (int32_t a = 0; a < out.n_axis; ++a) {
		const Pair &p = want[(size_t)a];
		const int32_t n = p.hi - p.lo;
		const std::vector<double> &zb = Z[(size_t)p.blk];
		out.eig.push_back(p.theta), out.resid.push_back(p.resid);
		for (int32_t i = 0; i < n; ++i) out.S[(size_t)a * m + (size_t)(p.lo + i)] = zb[(size_t)i * n + p.col];
	}
	return 0;
}

} // namespace pcoa

#ifdef __HIPCC__

constexpr int32_t PCOA_MAX_COL = 16384, PCOA_MAX_AXIS = 16;

struct PcoaBuf { enum { Q, V, X, Y, C, AB, STATE, S, OUT, N_BUF }; enum { H_STEP, H_OUT }; }; // page-locked: a chunk's alpha, beta and state; the results
static_assert(PcoaBuf::N_BUF <= PAN_MAX_DEV, "the pool has no room for the principal coordinates buffers");

template <int B> static void pcoa_mult_launch(hipStream_t st, const int32_t *q, int32_t N, int32_t ld, double scale, const double *x, double *y, const PcoaState *state)
{
	hipLaunchKernelGGL(k_pcoa_mult<B>, dim3((unsigned)((N + PC_ROWS - 1) / PC_ROWS)), dim3(BLOCK), 0, st, q, N, ld, scale, x, y, state);
}
static void pcoa_mult(int32_t b, hipStream_t st, const int32_t *q, int32_t N, int32_t ld, double scale, const double *x, double *y, const PcoaState *state)
{
	switch (b) {
	case 1: pcoa_mult_launch<1>(st, q, N, ld, scale, x, y, state); break;
	case 2: pcoa_mult_launch<2>(st, q, N, ld, scale, x, y, state); break;
	case 3: pcoa_mult_launch<3>(st, q, N, ld, scale, x, y, state); break;
	case 4: pcoa_mult_launch<4>(st, q, N, ld, scale, x, y, state); break;
	case 5: pcoa_mult_launch<5>(st, q, N, ld, scale, x, y, state); break;
	case 6: pcoa_mult_launch<6>(st, q, N, ld, scale, x, y, state); break;
	case 7: pcoa_mult_launch<7>(st, q, N, ld, scale, x, y, state); break;
	default: pcoa_mult_launch<8>(st, q, N, ld, scale, x, y, state); break;
	}
}

namespace {
// the Ops of pcoa::lanczos on the device.  V[max_vec + 1][ld]: row j is v_j, and w of step j is row j + 1
struct PcoaDev {
	PanDev &m;
	hipStream_t st;
	int32_t N, ld;
	double scale;
	uint32_t seed;
	const int32_t *d_q;
	double *d_V, *d_c, *d_ab, *h_step;
	PcoaState *d_state;
	bool timing;
	std::vector<hipEvent_t> ev; // PANGENE_PCOA_TIMING: a pair around every product
	double *row(int32_t j) const { return d_V + (size_t)j * (size_t)ld; }
	unsigned n_grid() const { return (unsigned)((N + BLOCK - 1) / BLOCK); }
	void mark()
	{
		if (!timing) return;
		hipEvent_t e = nullptr;
		if (hipEventCreate(&e) == hipSuccess) { (void)hipEventRecord(e, st); ev.push_back(e); }
	}
	// two passes of classical Gram-Schmidt of row j against the rows before it; the coefficients stay in c1 = d_c, c2 = d_c + PC_MAX_VEC + 1
	void orthogonalise(int32_t j)
	{
		if (j == 0) return;
		for (int pass = 0; pass < 2; ++pass) {
			double *c = d_c + (size_t)pass * (PC_MAX_VEC + 1);
			hipLaunchKernelGGL(k_pcoa_dots, dim3((unsigned)j), dim3(BLOCK), 0, st, d_V, ld, N, row(j), c, d_state);
			hipLaunchKernelGGL(k_pcoa_update, dim3(n_grid()), dim3(BLOCK), 0, st, d_V, ld, N, j, c, row(j), d_state);
		}
	}
	int start(int32_t j, uint32_t restart)
	{
		PANCHK(m, hipMemsetAsync(d_state, 0, sizeof(PcoaState), st)); // (the estimate of |B| comes back with the next chunk)
		hipLaunchKernelGGL(k_pcoa_start, dim3(n_grid()), dim3(BLOCK), 0, st, row(j), N, seed, restart);
		hipLaunchKernelGGL(k_pcoa_center, dim3(1), dim3(BLOCK), 0, st, row(j), N, 1, d_state);
		orthogonalise(j);
		hipLaunchKernelGGL(k_pcoa_norm, dim3(1), dim3(BLOCK), 0, st, row(j), N, -1, d_c, d_c, 0.0, d_ab, d_ab, d_state);
		PANCHK(m, hipGetLastError());
		return 0;
	}
	int steps(int32_t j0, int32_t nb, double est, double *alpha, double *beta, int32_t *n_done, int32_t *broke)
	{
		for (int32_t j = j0; j < j0 + nb; ++j) {
			mark();
			pcoa_mult(1, st, d_q, N, ld, scale, row(j), row(j + 1), d_state);
			mark();
			hipLaunchKernelGGL(k_pcoa_center, dim3(1), dim3(BLOCK), 0, st, row(j + 1), N, 1, d_state);
			orthogonalise(j + 1);
			hipLaunchKernelGGL(k_pcoa_norm, dim3(1), dim3(BLOCK), 0, st, row(j + 1), N, j, d_c, d_c + (PC_MAX_VEC + 1), est, d_ab, d_ab + PC_MAX_VEC, d_state);
		}
		PANCHK(m, hipGetLastError());
		// one small copy and the chunk's one wait: alpha and beta of the chunk, then the state
		PANCHK(m, hipMemcpyAsync(h_step, d_ab + j0, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, st));
		PANCHK(m, hipMemcpyAsync(h_step + pcoa::PC_CHUNK, d_ab + PC_MAX_VEC + j0, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, st));
		PANCHK(m, hipMemcpyAsync(h_step + 2 * pcoa::PC_CHUNK, d_state, sizeof(PcoaState), hipMemcpyDeviceToHost, st));
		PANCHK(m, hipStreamSynchronize(st));
		const PcoaState now = *(const PcoaState *)(h_step + 2 * pcoa::PC_CHUNK);
		if (now.broke == 2) return PGA_ERR_INVARIANT; // the start vector vanished: nothing is left to start from
		if (now.n_done < 0 || now.n_done > nb) return PGA_ERR_INVARIANT;
		for (int32_t s = 0; s < now.n_done; ++s) alpha[j0 + s] = h_step[s], beta[j0 + s] = h_step[pcoa::PC_CHUNK + s];
		*n_done = now.n_done, *broke = now.broke;
		PANCHK(m, hipMemsetAsync(&d_state->n_done, 0, sizeof(int32_t), st));
		return 0;
	}
};
}

extern "C" int pga_pan_pcoa(const pga_pcoa_in_t *in, pga_pcoa_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	memset(out, 0, sizeof(*out));
	if (in == nullptr || in->n < 1 || in->fbits < 0 || in->fbits > 30 || in->n_test < 0 || in->n_test > PC_MAX_B) return PGA_ERR_ARG;
	if (in->n > PCOA_MAX_COL || in->n_axis < 1 || in->n_axis > PCOA_MAX_AXIS) return PGA_ERR_RANGE; // (before anything is looked at or launched)
	if (in->q == nullptr || (in->n_test > 0 && (in->x_test == nullptr || in->y_test == nullptr))) return PGA_ERR_ARG;
	const int32_t N = in->n, ld = (N + 3) & ~3, nt = in->n_test;
	const int32_t k = std::min(in->n_axis, N - 1), max_step = in->max_step >= 1 ? std::min(in->max_step, PC_MAX_VEC) : PC_MAX_VEC;
	const int32_t max_vec = std::min(max_step, std::max(N - 1, 1));
	PanDev &m = g_pan[PAN_PCOA];
	std::lock_guard<std::mutex> lk(m.mu);
	double *h_step = m.get_host<double>(PcoaBuf::H_STEP, 2 * pcoa::PC_CHUNK + 2);
	double *h_out = m.get_host<double>(PcoaBuf::H_OUT, std::max((size_t)2 * PCOA_MAX_AXIS + (size_t)N * (size_t)std::max(k, 1), (size_t)N * (size_t)PC_MAX_B));
	PANMEM(h_step); PANMEM(h_out);
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	int32_t *d_q = m.get<int32_t>(PcoaBuf::Q, (size_t)N * (size_t)ld);
	double *d_V = m.get<double>(PcoaBuf::V, (size_t)(max_vec + 1) * (size_t)ld);
	double *d_x = m.get<double>(PcoaBuf::X, (size_t)ld * (size_t)PC_MAX_B), *d_y = m.get<double>(PcoaBuf::Y, (size_t)N * (size_t)std::max(PC_MAX_B, PCOA_MAX_AXIS));
	double *d_c = m.get<double>(PcoaBuf::C, 2 * (size_t)(PC_MAX_VEC + 1)), *d_ab = m.get<double>(PcoaBuf::AB, 2 * (size_t)PC_MAX_VEC);
	PcoaState *d_state = m.get<PcoaState>(PcoaBuf::STATE, 1);
	double *d_S = m.get<double>(PcoaBuf::S, (size_t)PCOA_MAX_AXIS * (size_t)PC_MAX_VEC);
	PANMEM(d_q); PANMEM(d_V); PANMEM(d_x); PANMEM(d_y); PANMEM(d_c); PANMEM(d_ab); PANMEM(d_state); PANMEM(d_S);
	// the rows of q padded to four columns, the padding zero; the padding of the vectors zero as well
	if (ld == N) PANCHK(m, hipMemcpyAsync(d_q, in->q, sizeof(int32_t) * (size_t)N * (size_t)N, hipMemcpyHostToDevice, st));
	else {
		PANCHK(m, hipMemsetAsync(d_q, 0, sizeof(int32_t) * (size_t)N * (size_t)ld, st));
		PANCHK(m, hipMemcpy2DAsync(d_q, sizeof(int32_t) * (size_t)ld, in->q, sizeof(int32_t) * (size_t)N, sizeof(int32_t) * (size_t)N, (size_t)N, hipMemcpyHostToDevice, st));
	}
	PANCHK(m, hipMemsetAsync(d_V, 0, sizeof(double) * (size_t)(max_vec + 1) * (size_t)ld, st));
	PANCHK(m, hipMemsetAsync(d_state, 0, sizeof(PcoaState), st));
	const double scale = -std::ldexp(1.0, -2 * in->fbits - 1);
	if (nt > 0) { // tests only: Y = A X - the column means, from the product kernel
		PANCHK(m, hipMemsetAsync(d_x, 0, sizeof(double) * (size_t)ld * (size_t)nt, st));
		PANCHK(m, hipMemcpyAsync(d_x, in->x_test, sizeof(double) * (size_t)N * (size_t)nt, hipMemcpyHostToDevice, st));
		pcoa_mult(nt, st, d_q, N, ld, scale, d_x, d_y, d_state);
		hipLaunchKernelGGL(k_pcoa_center, dim3((unsigned)nt), dim3(BLOCK), 0, st, d_y, N, nt, d_state);
		PANCHK(m, hipGetLastError());
		PANCHK(m, hipMemcpyAsync(h_out, d_y, sizeof(double) * (size_t)N * (size_t)nt, hipMemcpyDeviceToHost, st));
		PANCHK(m, hipStreamSynchronize(st));
		memcpy(in->y_test, h_out, sizeof(double) * (size_t)N * (size_t)nt);
	}
	out->eig = h_out, out->resid = h_out + PCOA_MAX_AXIS, out->vec = h_out + 2 * PCOA_MAX_AXIS;
	if (k < 1) return 0; // one assembly: the centred subspace is empty
	PcoaDev dev{m, st, N, ld, scale, in->seed, d_q, d_V, d_c, d_ab, h_step, d_state, getenv("PANGENE_PCOA_TIMING") != nullptr, {}};
	pcoa::Result r;
	const int rc = pcoa::lanczos(dev, N, k, max_step, r);
	float mult_ms = 0;
	for (size_t i = 0; i + 1 < dev.ev.size(); i += 2) { float ms = 0; if (hipEventElapsedTime(&ms, dev.ev[i], dev.ev[i + 1]) == hipSuccess) mult_ms += ms; }
	for (hipEvent_t e : dev.ev) (void)hipEventDestroy(e);
	if (rc != 0) return rc;
	if (r.n_axis > 0) { // the Ritz vectors X = V S
		PANCHK(m, hipMemcpyAsync(d_S, r.S.data(), sizeof(double) * (size_t)r.n_axis * (size_t)r.n_step, hipMemcpyHostToDevice, st));
		hipLaunchKernelGGL(k_pcoa_ritz, dim3((unsigned)((N + BLOCK - 1) / BLOCK), (unsigned)r.n_axis), dim3(BLOCK), 0, st, d_V, ld, N, r.n_step, d_S, r.n_axis, d_y);
		PANCHK(m, hipGetLastError());
		PANCHK(m, hipMemcpyAsync(h_out + 2 * PCOA_MAX_AXIS, d_y, sizeof(double) * (size_t)N * (size_t)r.n_axis, hipMemcpyDeviceToHost, st));
		PANCHK(m, hipStreamSynchronize(st));
	}
	for (int32_t a = 0; a < r.n_axis; ++a) h_out[a] = r.eig[(size_t)a], h_out[PCOA_MAX_AXIS + a] = r.resid[(size_t)a];
	out->n_axis = r.n_axis, out->n_step = r.n_step, out->n_restart = r.n_restart, out->converged = r.converged;
	if (dev.timing)
		fprintf(stderr, "[pcoa-kernels] assemblies=%d axes=%d steps=%d restarts=%d converged=%d mult_ms=%.3f mult_ms_per_step=%.4f\n", N, r.n_axis, r.n_step, r.n_restart,
		        r.converged, mult_ms, r.n_step ? mult_ms / r.n_step : 0.0);
	return 0;
}

#endif // __HIPCC__
