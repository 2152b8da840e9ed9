// pan_rates.hpp -- maximum-likelihood gene gain and loss rates on the tree of the assemblies (pg_rates_file, pg_write_rates,
// pg_pan_rates, pangene rates; DESIGN.md section 8 "Gain and loss rates"): a two-state Markov model per item on the tree with its branch
// lengths, corrected for the items nobody can observe.  Both builds share the branch lengths, the tables (expm1 lives here, never in a
// kernel), the lattice search, the logarithms and the sum of the log-likelihood, the rate scan and the text.  The likelihoods of a batch
// of parameter sets and the posteriors come from the backend (pga_pan_rates: the tree as pan_gainloss.hpp's postfix program), or, when
// the backend has no such entry, from the plain loops below, node by node in join order over the records' tree: the second
// implementation, with the same power-of-two rescaling rule.

namespace pgx {
namespace {

constexpr double RATES_T_FLOOR = 1.0 / 1048576.0; // 2^-20: the shortest normalised branch
constexpr double RATES_MIN = 1e-9, RATES_MAX = 1e9; // what -g and -l take
constexpr int32_t RATES_MOVES = 16;                // lattice rounds that may repeat at the same step

// The raw branch lengths of the records by newick()'s formulas, in record units and node id order (pairs_tree: leaf x = x, join t =
// A + t); the root's is 0.  NJ's root sits in the middle of z's branch.  A >= 2
void rates_lengths(const int64_t *rec, int32_t A, int32_t method, const std::vector<int32_t> &kid, std::vector<double> &len)
{
	const size_t n_join = kid.size() / 2;
	len.assign((size_t)A + n_join, 0.0);
	if (A == 2) { len[0] = len[1] = 0.5; return; }
	if (method == PG_TREE_NJ) {
		const size_t n_plain = (size_t)A - 3;
		for (size_t t = 0; t < n_plain; ++t) {
			const int64_t *r = rec + 6 * t;
			const double li = ((double)r[2] + (double)(r[3] - r[4]) / (double)(r[5] - 2)) / 2.0, lj = (double)r[2] - li;
			len[(size_t)kid[2 * t]] = li, len[(size_t)kid[2 * t + 1]] = lj;
		}
		const int64_t *r = rec + 6 * n_plain;
		const double lx = (double)(r[3] + r[4] - r[5]) / 2.0, ly = (double)(r[3] + r[5] - r[4]) / 2.0, lz = (double)(r[4] + r[5] - r[3]) / 2.0;
		len[(size_t)kid[2 * n_plain]] = lx, len[(size_t)kid[2 * n_plain + 1]] = ly;
		len[(size_t)kid[2 * n_plain + 2]] = lz / 2.0, len[(size_t)kid[2 * n_plain + 3]] = lz / 2.0; // the (x, y) node and z
		return;
	}
	std::vector<double> height((size_t)A + n_join, 0.0);
	for (size_t t = 0; t < n_join; ++t) {
		const double h = (double)rec[6 * t + 2] / 2.0;
		for (size_t c = 0; c < 2; ++c) len[(size_t)kid[2 * t + c]] = h - height[(size_t)kid[2 * t + c]];
		height[(size_t)A + t] = h;
	}
}

// len -> t (normalised, floored; the root's stays 0); returns T, the sum of max(len, 0)
double rates_normalise(const std::vector<double> &len, std::vector<double> &t)
{
	double T = 0;
	for (size_t v = 0; v + 1 < len.size(); ++v) T += std::max(len[v], 0.0);
	t.assign(len.size(), 0.0);
	if (!(T > 0)) return T;
	for (size_t v = 0; v + 1 < len.size(); ++v) t[v] = std::max(std::max(len[v], 0.0) / T, RATES_T_FLOOR);
	return T;
}

// P00 P01 P10 P11 of a branch of length t under (lambda, mu); pi[2]
inline void rates_row(double lambda, double mu, double t, double *p)
{
	const double s = lambda + mu, pi1 = lambda / s, pi0 = mu / s, q = -std::expm1(-s * t);
	p[1] = pi1 * q, p[0] = 1.0 - p[1], p[2] = pi0 * q, p[3] = 1.0 - p[2];
}
inline void rates_pi(double lambda, double mu, double *pi) { const double s = lambda + mu; pi[0] = mu / s, pi[1] = lambda / s; }

// the larger of two non-negative values decides the exponent both lose (frexp / ldexp: exact); returns it
inline int rates_rescale(double &a, double &b)
{
	const double big = std::max(a, b);
	if (!(big > 0) || !std::isfinite(big)) return 0;
	int e;
	(void)std::frexp(big, &e);
	a = std::ldexp(a, -e), b = std::ldexp(b, -e);
	return e;
}

// What one evaluation returns: lik_m / lik_e[n_set][n], L = m 2^e; with post, for set 0, gene[n][3] = gains, losses, root and
// node[n_node][3] = present, gains, losses in node id order, summed over the items [0, n_sum)
struct RatesOut { std::vector<double> lik_m, gene, node; std::vector<int32_t> lik_e; };

// The second implementation: plain loops over the tree itself.  bits[A][W] over n items; par[n_set][2] = lambda, mu; t[n_node]
void rates_host(const uint32_t *bits, int32_t n, int32_t A, const std::vector<int32_t> &kid, const std::vector<double> &t, const double *par, int32_t n_set, bool post,
                int32_t n_sum, RatesOut &o)
{
	const size_t W = ((size_t)n + 31) / 32, n_join = kid.size() / 2, n_node = (size_t)A + n_join, root = n_node - 1;
	o.lik_m.assign((size_t)n_set * (size_t)n, 0.0), o.lik_e.assign((size_t)n_set * (size_t)n, 0);
	if (post) o.gene.assign(3 * (size_t)n, 0.0), o.node.assign(3 * n_node, 0.0);
	std::vector<double> P(4 * n_node), in(2 * n_node), out(2 * n_node);
	std::vector<int64_t> E(n_node);
	for (int32_t s = 0; s < n_set; ++s) {
		double pi[2];
		rates_pi(par[2 * s], par[2 * s + 1], pi);
		for (size_t v = 0; v < root; ++v) rates_row(par[2 * s], par[2 * s + 1], t[v], &P[4 * v]);
		for (int32_t i = 0; i < n; ++i) {
			for (int32_t x = 0; x < A; ++x) {
				const uint32_t b = item_bit(bits, W, x, i);
				in[2 * (size_t)x] = b ? 0.0 : 1.0, in[2 * (size_t)x + 1] = b ? 1.0 : 0.0, E[(size_t)x] = 0;
			}
			for (size_t j = 0; j < n_join; ++j) {
				const size_t v = (size_t)A + j, c = (size_t)kid[2 * j], d = (size_t)kid[2 * j + 1];
				double a0 = (P[4 * c] * in[2 * c] + P[4 * c + 1] * in[2 * c + 1]) * (P[4 * d] * in[2 * d] + P[4 * d + 1] * in[2 * d + 1]);
				double a1 = (P[4 * c + 2] * in[2 * c] + P[4 * c + 3] * in[2 * c + 1]) * (P[4 * d + 2] * in[2 * d] + P[4 * d + 3] * in[2 * d + 1]);
				E[v] = E[c] + E[d] + rates_rescale(a0, a1);
				in[2 * v] = a0, in[2 * v + 1] = a1;
			}
			const double L = pi[0] * in[2 * root] + pi[1] * in[2 * root + 1];
			int e = 0;
			const double m = L > 0 ? std::frexp(L, &e) : 0.0;
			o.lik_m[(size_t)s * (size_t)n + (size_t)i] = m, o.lik_e[(size_t)s * (size_t)n + (size_t)i] = L > 0 ? (int32_t)(E[root] + e) : 0;
			if (!post || s != 0) continue;
			const bool counts = i < n_sum;
			double *g = &o.gene[3 * (size_t)i];
			g[2] = L > 0 ? pi[1] * in[2 * root + 1] / L : 0.0;
			if (counts) o.node[3 * root] += g[2];
			out[2 * root] = pi[0], out[2 * root + 1] = pi[1];
			for (size_t j = n_join; j-- > 0;) {
				const size_t v = (size_t)A + j;
				for (size_t side = 0; side < 2; ++side) {
					const size_t c = (size_t)kid[2 * j + side], d = (size_t)kid[2 * j + 1 - side];
					const double O0 = out[2 * v] * (P[4 * d] * in[2 * d] + P[4 * d + 1] * in[2 * d + 1]);
					const double O1 = out[2 * v + 1] * (P[4 * d + 2] * in[2 * d] + P[4 * d + 3] * in[2 * d + 1]);
					const double J00 = O0 * P[4 * c] * in[2 * c], J01 = O0 * P[4 * c + 1] * in[2 * c + 1], J10 = O1 * P[4 * c + 2] * in[2 * c], J11 = O1 * P[4 * c + 3] * in[2 * c + 1];
					const double Z = (J00 + J01) + (J10 + J11);
					const double present = Z > 0 ? (J01 + J11) / Z : 0.0, gain = Z > 0 ? J01 / Z : 0.0, loss = Z > 0 ? J10 / Z : 0.0;
					double o0 = O0 * P[4 * c] + O1 * P[4 * c + 2], o1 = O0 * P[4 * c + 1] + O1 * P[4 * c + 3];
					(void)rates_rescale(o0, o1);
					out[2 * c] = o0, out[2 * c + 1] = o1;
					g[0] += gain, g[1] += loss;
					if (counts) o.node[3 * c] += present, o.node[3 * c + 1] += gain, o.node[3 * c + 2] += loss;
				}
			}
		}
	}
}

double t_rates_fit = 0, t_rates_post = 0; // seconds of the evaluations of the last command: the search; the posteriors and the scan

// The model over one set of items: the tree, the normalised lengths, the items with the all-absent pseudo-item behind them, and the
// route the evaluations take.
struct RatesModel {
	int32_t A = 0, n = 0; // n: the items, the pseudo-item (the last) included
	std::vector<int32_t> kid;
	std::vector<double> t;
	std::vector<uint32_t> bits; // [A][W] over the n items, in assembly order
	// the backend's view
	const pga_backend_t *be = nullptr;
	std::vector<uint8_t> op;
	std::vector<int32_t> node_of, par;
	std::vector<uint32_t> rows;
	std::vector<double> tab, pi;

	int prepare()
	{
		be = backend_default();
		if (be->pan_rates == nullptr) return 0;
		const size_t W = ((size_t)n + 31) / 32;
		if (gainloss_program(bits, W, A, kid, op, node_of, par, rows) > GAINLOSS_DEPTH) return PGA_ERR_RANGE; // (out of reach below 65 536 leaves)
		return 0;
	}
	// par[n_set][2] = lambda, mu
	int eval(const double *par_, int32_t n_set, bool post, RatesOut &o)
	{
		const size_t n_node = t.size();
		if (be->pan_rates == nullptr) { rates_host(bits.data(), n, A, kid, t, par_, n_set, post, n - 1, o); return 0; }
		tab.resize((size_t)n_set * n_node * 4), pi.resize(2 * (size_t)n_set);
		for (int32_t s = 0; s < n_set; ++s) {
			rates_pi(par_[2 * s], par_[2 * s + 1], &pi[2 * (size_t)s]);
			for (size_t k = 0; k < n_node; ++k) rates_row(par_[2 * s], par_[2 * s + 1], t[(size_t)node_of[k]], &tab[((size_t)s * n_node + k) * 4]);
		}
		const pga_rates_in_t in{op.data(), rows.data(), par.data(), n, A, n_set, tab.data(), pi.data(), post ? 1 : 0, n - 1, nullptr};
		pga_rates_out_t res{};
		const int rc = be->pan_rates(&in, &res);
		if (rc != 0) return rc;
		o.lik_m.assign(res.lik_m, res.lik_m + (size_t)n_set * (size_t)n), o.lik_e.assign(res.lik_e, res.lik_e + (size_t)n_set * (size_t)n);
		if (post) {
			o.gene.assign(res.gene, res.gene + 3 * (size_t)n);
			o.node.assign(3 * n_node, 0.0);
			for (size_t k = 0; k < n_node; ++k) std::memcpy(&o.node[3 * (size_t)node_of[k]], res.node + 3 * k, sizeof(double) * 3);
		}
		return 0;
	}
};

inline double rates_ln(double m, int32_t e) { return std::log(m) + (double)e * 0.6931471805599453094; }

// ll[i] = ln L_i - ln(1 - L_0) of set s for the items but the last, which is the pseudo-item; returns LL, summed in ascending order
double rates_ll(const RatesOut &o, int32_t s, int32_t n, double *ll = nullptr)
{
	const double *m = &o.lik_m[(size_t)s * (size_t)n];
	const int32_t *e = &o.lik_e[(size_t)s * (size_t)n];
	const double corr = std::log1p(-std::ldexp(m[n - 1], e[n - 1]));
	double sum = 0;
	for (int32_t i = 0; i + 1 < n; ++i) {
		const double l = rates_ln(m[i], e[i]);
		sum += l;
		if (ll != nullptr) ll[i] = l - corr;
	}
	return sum - (double)(n - 1) * corr;
}

struct RatesFit { double lambda = 0, mu = 0, LL = 0; int32_t rounds = 0, converged = 1; };

// The lattice search in (log2 lambda, log2 mu): 25 parameter sets a round, ONE evaluation a round
int rates_search(RatesModel &mod, RatesFit &fit)
{
	double cx = 0, cy = 0, h = 2.0, par[50];
	int32_t moves = 0;
	RatesOut o;
	for (;;) {
		for (int i = 0; i < 5; ++i)
			for (int j = 0; j < 5; ++j) par[2 * (5 * i + j)] = std::exp2(cx + (i - 2) * h), par[2 * (5 * i + j) + 1] = std::exp2(cy + (j - 2) * h);
		const int rc = mod.eval(par, 25, false, o);
		if (rc != 0) return rc;
		++fit.rounds;
		int best = 0;
		double best_ll = rates_ll(o, 0, mod.n);
		for (int s = 1; s < 25; ++s) {
			const double ll = rates_ll(o, s, mod.n);
			if (ll > best_ll) best = s, best_ll = ll; // a tie keeps the lowest i, then the lowest j
		}
		const int bi = best / 5, bj = best % 5;
		cx = std::min(std::max(cx + (bi - 2) * h, -20.0), 20.0), cy = std::min(std::max(cy + (bj - 2) * h, -20.0), 20.0);
		const bool edge = bi == 0 || bi == 4 || bj == 0 || bj == 4;
		if (edge && moves < RATES_MOVES) { ++moves; continue; }
		if (h <= 1.0 / 1024.0) break;
		h /= 2;
	}
	fit.lambda = std::exp2(cx), fit.mu = std::exp2(cy);
	fit.converged = !(std::fabs(cx) >= 20.0 || std::fabs(cy) >= 20.0 || moves >= RATES_MOVES);
	return 0;
}

bool rates_rate_ok(double gain, double loss)
{
	if (gain == 0 && loss == 0) return true;
	return gain >= RATES_MIN && gain <= RATES_MAX && loss >= RATES_MIN && loss <= RATES_MAX;
}

bool rates_opt_ok(const pg_rates_opt_t *o)
{
	return o != nullptr && (o->type == PG_DIST_GENE || o->type == PG_DIST_ADJ) && (o->metric == PG_DIST_JACCARD || o->metric == PG_DIST_DIFF) &&
	       (o->method == PG_TREE_NJ || o->method == PG_TREE_UPGMA) && (o->out == PG_GAINLOSS_GENE || o->out == PG_GAINLOSS_NODE) && rates_rate_ok(o->gain, o->loss) &&
	       o->min_changes >= 0; // (a NaN fails every comparison)
}

// bits[A][W] over M items, the tree of kid with the raw lengths len: fit[6] = lambda, mu, LL, rounds, converged, T; gene[M][7] = lnL,
// gains, losses, root, rate, LRT, p_rate (NaN for an item absent everywhere); node[2 A - 1][4] = length, present, gains, losses in node
// id order; present[M].  Returns 0, a PGA_ERR_* code, or 1: no model (A < 2 or T = 0), fit[5] = T alone is set
int rates_core(const std::vector<uint32_t> &bits, int32_t M, int32_t A, const std::vector<int32_t> &kid, const std::vector<double> &len, double gain, double loss, double *fit,
               double *gene, double *node, std::vector<int32_t> &present, int32_t *n_used)
{
	const double nan = std::nan("");
	std::fill(fit, fit + 6, nan);
	fit[3] = fit[4] = 0;
	std::fill(gene, gene + 7 * (size_t)M, nan);
	std::fill(node, node + 4 * (size_t)std::max(2 * A - 1, 0), 0.0);
	item_counts(bits.data(), M, A, present);
	RatesModel mod;
	const double T = A >= 2 ? rates_normalise(len, mod.t) : 0.0;
	fit[5] = T;
	*n_used = 0;
	if (A < 2 || !(T > 0)) return 1;
	if (A > GAINLOSS_MAX_LEAF || M >= GAINLOSS_MAX_ITEM) return PGA_ERR_RANGE;
	// the items present somewhere, in their order, and the all-absent pseudo-item behind them
	std::vector<int32_t> used;
	for (int32_t i = 0; i < M; ++i) if (present[(size_t)i] > 0) used.push_back(i);
	const int32_t G = (int32_t)used.size();
	*n_used = G;
	const size_t W = ((size_t)M + 31) / 32, Wc = ((size_t)G + 1 + 31) / 32;
	mod.A = A, mod.n = G + 1, mod.kid = kid;
	mod.bits.assign((size_t)A * Wc, 0);
	if (G == M) {
		for (int32_t a = 0; a < A && W > 0; ++a) std::memcpy(&mod.bits[(size_t)a * Wc], &bits[(size_t)a * W], sizeof(uint32_t) * W);
	} else {
		std::vector<int32_t> at((size_t)M, -1);
		for (int32_t k = 0; k < G; ++k) at[(size_t)used[(size_t)k]] = k;
		for (int32_t a = 0; a < A; ++a)
			for (size_t w = 0; w < W; ++w)
				for (uint32_t x = bits[(size_t)a * W + w]; x != 0; x &= x - 1) {
					const int32_t k = at[32 * w + (size_t)__builtin_ctz(x)];
					mod.bits[(size_t)a * Wc + (size_t)(k >> 5)] |= 1u << (k & 31);
				}
	}
	for (size_t v = 0; v < mod.t.size(); ++v) node[4 * v] = mod.t[v];
	if (G == 0) return 1; // nothing to fit
	int rc = mod.prepare();
	if (rc != 0) return rc;
	RatesFit f;
	const double t0 = now_sec();
	if (gain > 0) f.lambda = gain, f.mu = loss;
	else if ((rc = rates_search(mod, f)) != 0) return rc;
	const double t1 = now_sec();
	t_rates_fit += t1 - t0;
	// the posteriors at the rates, then the scan of nine multipliers
	RatesOut post, scan;
	const double at[2] = {f.lambda, f.mu};
	if ((rc = mod.eval(at, 1, true, post)) != 0) return rc;
	f.LL = rates_ll(post, 0, mod.n);
	double par[18];
	for (int r = 0; r < 9; ++r) par[2 * r] = std::ldexp(f.lambda, r - 4), par[2 * r + 1] = std::ldexp(f.mu, r - 4);
	if ((rc = mod.eval(par, 9, false, scan)) != 0) return rc;
	std::vector<double> ll(9 * (size_t)G);
	for (int r = 0; r < 9; ++r) (void)rates_ll(scan, r, mod.n, &ll[(size_t)r * (size_t)G]);
	static const int order[9] = {4, 3, 5, 2, 6, 1, 7, 0, 8}; // nearer 1 first, then the smaller
	for (int32_t k = 0; k < G; ++k) {
		int best = 4;
		for (const int r : order) if (ll[(size_t)r * (size_t)G + (size_t)k] > ll[(size_t)best * (size_t)G + (size_t)k]) best = r;
		double *o = gene + 7 * (size_t)used[(size_t)k];
		const double lrt = std::max(2.0 * (ll[(size_t)best * (size_t)G + (size_t)k] - ll[4 * (size_t)G + (size_t)k]), 0.0);
		o[0] = ll[4 * (size_t)G + (size_t)k], o[1] = post.gene[3 * (size_t)k], o[2] = post.gene[3 * (size_t)k + 1], o[3] = post.gene[3 * (size_t)k + 2];
		o[4] = std::ldexp(1.0, best - 4), o[5] = lrt, o[6] = std::erfc(std::sqrt(lrt / 2.0));
	}
	for (size_t v = 0; v < mod.t.size(); ++v) node[4 * v + 1] = post.node[3 * v], node[4 * v + 2] = post.node[3 * v + 1], node[4 * v + 3] = post.node[3 * v + 2];
	t_rates_post += now_sec() - t1;
	fit[0] = f.lambda, fit[1] = f.mu, fit[2] = f.LL, fit[3] = f.rounds, fit[4] = f.converged;
	return 0;
}

// the items, the tree of all assemblies with its lengths, the fit, one of the two tables
int rates_run(const ItemSource &src, const pg_rates_opt_t *o)
{
	const double t_start = now_sec();
	if (!rates_opt_ok(o) || (o->gain > 0) != (o->loss > 0)) return PGA_ERR_ARG;
	std::vector<std::string> names, item;
	std::vector<uint32_t> bits;
	int32_t M = 0;
	if (src(o->type, names, bits, M, &item) != 0) return PAN_NO_ITEMS;
	const int32_t A = (int32_t)names.size();
	const double t_prep = now_sec() - t_start;
	OutBuf ob;
	std::string &s = ob.s;
	s = o->out == PG_GAINLOSS_GENE ? "Gene\tPresent\tlnL\tGains\tLosses\tChanges\tRoot\tRate\tLRT\tp_rate\n" : "Node\tChild1\tChild2\tLeaves\tLength\tPresent\tGains\tLosses\n";
	if (A < 2 || M == 0) {
		ob.finish();
		std::fprintf(stderr, "[M::pan_rates] fewer than two assemblies or no items: no model\n");
		return 0;
	}
	if (A > GAINLOSS_MAX_LEAF || M >= GAINLOSS_MAX_ITEM) return PGA_ERR_RANGE;
	std::vector<int64_t> rec((size_t)6 * (size_t)A);
	std::vector<int32_t> q;
	int32_t F = 0;
	int rc = A >= 3 ? tree_records(bits, M, A, o->metric, o->method, q, rec.data(), &F) : 0;
	if (rc != 0) return rc;
	std::vector<int32_t> kid;
	if (!pairs_tree(rec.data(), A, o->method, kid)) return PGA_ERR_ARG;
	std::vector<double> len;
	rates_lengths(rec.data(), A, o->method, kid, len);
	const size_t n_node = (size_t)A + kid.size() / 2;
	std::vector<double> gene(7 * (size_t)M), node(4 * n_node);
	std::vector<int32_t> present;
	double fit[6];
	int32_t G = 0;
	t_rates_fit = t_rates_post = 0;
	rc = rates_core(bits, M, A, kid, len, o->gain, o->loss, fit, gene.data(), node.data(), present, &G);
	if (rc == 1) {
		ob.finish();
		std::fprintf(stderr, "[M::pan_rates] %s: no model\n", fit[5] > 0 ? "no item is present anywhere" : "the tree has no length (all assemblies are identical)");
		return 0;
	}
	if (rc != 0) return rc;
	char b[512];
	std::snprintf(b, sizeof(b), "#\titems=%s\tmetric=%s\tmethod=%s\tA=%d\tG=%d\tgain=%.6g\tloss=%.6g\tlnL=%.6g\trounds=%d\tconverged=%d\ttreelen=%.6g\n",
	              o->type == PG_DIST_GENE ? "gene" : "adj", o->metric == PG_DIST_JACCARD ? "jaccard" : "diff", o->method == PG_TREE_NJ ? "nj" : "upgma", A, G, fit[0], fit[1], fit[2],
	              (int)fit[3], (int)fit[4], std::ldexp(fit[5], -F));
	s += b;
	if (o->out == PG_GAINLOSS_GENE) {
		for (size_t i = 0; i < (size_t)M; ++i) {
			const double *r = gene.data() + 7 * i;
			if (present[i] == 0 || r[1] + r[2] < o->min_changes) continue;
			std::snprintf(b, sizeof(b), "\t%d\t%.6g\t%.6g\t%.6g\t%.6g\t%.6g\t%.6g\t%.6g\t%.6g\n", present[i], r[0], r[1], r[2], r[1] + r[2], r[3], r[4], r[5], r[6]);
			s += item[i], s += b;
			ob.flush_if_full();
		}
	} else {
		std::vector<int32_t> leaves(n_node, 1);
		for (size_t t = 0; t < kid.size() / 2; ++t) leaves[(size_t)A + t] = leaves[(size_t)kid[2 * t]] + leaves[(size_t)kid[2 * t + 1]];
		auto name_of = [&](size_t v) { return v < (size_t)A ? names[v] : "@" + std::to_string(v - (size_t)A); };
		for (size_t v = 0; v < n_node; ++v) {
			s += name_of(v), s += '\t';
			if (v < (size_t)A) s += ".\t.";
			else s += name_of((size_t)kid[2 * (v - (size_t)A)]), s += '\t', s += name_of((size_t)kid[2 * (v - (size_t)A) + 1]);
			const double *r = node.data() + 4 * v;
			if (v + 1 == n_node) std::snprintf(b, sizeof(b), "\t%d\t%.6g\t%.6g\tNA\tNA\n", leaves[v], r[0], r[1]);
			else std::snprintf(b, sizeof(b), "\t%d\t%.6g\t%.6g\t%.6g\t%.6g\n", leaves[v], r[0], r[1], r[2], r[3]);
			s += b;
			ob.flush_if_full();
		}
	}
	ob.finish();
	if (std::getenv("PANGENE_RATES_TIMING") != nullptr)
		std::fprintf(stderr, "[rates-timing] route=%s items=%d assemblies=%d rounds=%d prep_ms=%.3f fit_ms=%.3f post_ms=%.3f all_ms=%.3f\n", src.route(), M, A, (int)fit[3],
		             t_prep * 1e3, t_rates_fit * 1e3, t_rates_post * 1e3, (now_sec() - t_start) * 1e3);
	return 0;
}

} // namespace
} // namespace pgx

extern "C" {

void pg_rates_opt_init(pg_rates_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->method = PG_TREE_UPGMA, o->out = PG_GAINLOSS_GENE, o->gain = 0, o->loss = 0, o->min_changes = 0;
}

int pg_rates_file(const char *gfa_fn, const pg_rates_opt_t *o)
{
	if (o == nullptr) { std::fprintf(stderr, "Error: pan_rates: no options\n"); return -2; }
	return file_result(rates_run(items_of_file(gfa_fn), o), gfa_fn, "pan_rates");
}

void pg_write_rates(pg_graph_t *q, const pg_rates_opt_t *o)
{
	if (o == nullptr) { set_error(PGA_ERR_ARG, "pg_write_rates"); return; }
	graph_result(rates_run(items_of_graph(q), o), "pg_write_rates");
}

int pg_pan_rates(const uint8_t *presence, int32_t n_item, int32_t n_asm, const int64_t *rec, int32_t method, const pg_rates_opt_t *o, double *fit_out, double *gene_out,
                 double *node_out)
{
	if (n_item < 0 || n_asm < 0 || (method != PG_TREE_NJ && method != PG_TREE_UPGMA) || (n_asm >= 3 && rec == nullptr) || o == nullptr) return PGA_ERR_ARG;
	if (!rates_rate_ok(o->gain, o->loss) || (o->gain > 0) != (o->loss > 0) || fit_out == nullptr) return PGA_ERR_ARG;
	if (((size_t)n_item * (size_t)n_asm > 0 && presence == nullptr) || (n_item > 0 && gene_out == nullptr) || (n_asm > 0 && node_out == nullptr)) return PGA_ERR_ARG;
	if (n_asm > GAINLOSS_MAX_LEAF || n_item >= GAINLOSS_MAX_ITEM) return PGA_ERR_RANGE;
	std::vector<int32_t> kid;
	if (!pairs_tree(rec, n_asm, method, kid)) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	std::vector<double> len;
	if (n_asm >= 2) rates_lengths(rec, n_asm, method, kid, len);
	std::vector<int32_t> present;
	int32_t G = 0;
	t_rates_fit = t_rates_post = 0;
	const int rc = rates_core(bits, n_item, n_asm, kid, len, o->gain, o->loss, fit_out, gene_out, node_out, present, &G);
	return rc == 1 ? 0 : rc;
}

} // extern "C"
