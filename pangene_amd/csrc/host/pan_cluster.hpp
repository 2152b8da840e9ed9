// pan_cluster.hpp -- clusters (pg_cluster_file, pg_write_cluster, pg_pan_medoids, pg_pan_cluster, pangene cluster; DESIGN.md section 8
// "Clusters"): k-medoids over the fixed-point distances of pan_tree.hpp, on the backend (pga_pan_medoids) or as the plain loops below; the
// silhouettes and the text are code both builds share.

namespace pgx {
namespace {

constexpr int32_t MED_IN_MAX = 1 << 29, MED_MAX_K = 1024;

struct Medoids { // what one run of k-medoids leaves (include/pangene_hip.h pga_medoids_out_t)
	std::vector<int32_t> medoid, label, dist, size;
	std::vector<int64_t> sums, rec;
	int64_t td = 0;
	int32_t n_swap = 0, converged = 0;
};

// q[n][n] as pg_pan_medoids checks it (symmetric, zero diagonal, entries in [0, 2^29)): 0, PGA_ERR_ARG or PGA_ERR_RANGE
int fixed_matrix_ok(const int32_t *q, int32_t n)
{
	const size_t N = (size_t)n;
	bool big = false;
	for (size_t i = 0; i < N; ++i) {
		if (q[i * N + i] != 0) return PGA_ERR_ARG;
		for (size_t j = i + 1; j < N; ++j) {
			if (q[i * N + j] != q[j * N + i] || q[i * N + j] < 0) return PGA_ERR_ARG;
			big |= q[i * N + j] >= MED_IN_MAX;
		}
	}
	return big ? PGA_ERR_RANGE : 0;
}

// k-medoids as the definition states it.  A delta is the difference of two TDs, each column's share formed directly: the column's distance
// after the exchange -- the smaller of d and its distance to the nearest medoid that stays -- minus its distance before.
void medoids_host(const int32_t *q, int32_t n, int32_t k, int32_t max_iter, Medoids &r)
{
	const size_t N = (size_t)n, K = (size_t)k;
	std::vector<int32_t> med, D(N, MED_IN_MAX), DS(N), NN(N);
	std::vector<uint8_t> in(N, 0);
	r.rec.clear();
	for (size_t s = 0; s < K; ++s) { // BUILD
		int64_t best = -1;
		size_t bx = 0;
		for (size_t x = 0; x < N; ++x) {
			if (in[x]) continue;
			int64_t g = 0;
			for (size_t o = 0; o < N; ++o) g += std::max(0, D[o] - q[x * N + o]);
			if (g > best) best = g, bx = x;
		}
		med.push_back((int32_t)bx), in[bx] = 1;
		for (size_t o = 0; o < N; ++o) D[o] = std::min(D[o], q[bx * N + o]);
		r.rec.insert(r.rec.end(), {(int64_t)bx, -1, best});
	}
	r.n_swap = 0, r.converged = 0;
	for (int32_t it = 0; it < max_iter; ++it) { // SWAP
		for (size_t o = 0; o < N; ++o) { // the nearest medoid's slot, its distance, and the distance to the nearest of the others
			int32_t d1 = MED_IN_MAX, d2 = MED_IN_MAX, nn = 0;
			for (size_t s = 0; s < K; ++s) {
				const int32_t d = q[(size_t)med[s] * N + o];
				if (d < d1) d2 = d1, d1 = d, nn = (int32_t)s;
				else if (d < d2) d2 = d;
			}
			D[o] = d1, DS[o] = d2, NN[o] = nn;
		}
		int64_t best = 0;
		size_t bx = 0, bs = 0;
		bool have = false;
		for (size_t x = 0; x < N; ++x) {
			if (in[x]) continue;
			const int32_t *row = q + x * N;
			for (size_t s = 0; s < K; ++s) {
				int64_t delta = 0;
				for (size_t o = 0; o < N; ++o) delta += std::min(row[o], NN[o] == (int32_t)s ? DS[o] : D[o]) - D[o];
				if (!have || delta < best || (delta == best && x == bx && med[s] < med[bs])) best = delta, bx = x, bs = s, have = true;
			}
		}
		if (best >= 0) { r.converged = 1; break; }
		r.rec.insert(r.rec.end(), {(int64_t)bx, (int64_t)med[bs], best});
		in[(size_t)med[bs]] = 0, in[bx] = 1, med[bs] = (int32_t)bx;
		++r.n_swap;
	}
	r.medoid = med;
	std::sort(r.medoid.begin(), r.medoid.end());
	r.label.assign(N, 0), r.dist.assign(N, 0), r.size.assign(K, 0), r.sums.assign(N * K, 0), r.td = 0;
	for (size_t c = 0; c < K; ++c) r.label[(size_t)r.medoid[c]] = -1 - (int32_t)c; // (marks the medoids)
	for (size_t o = 0; o < N; ++o) {
		if (r.label[o] < 0) r.label[o] = -1 - r.label[o];
		else {
			int32_t d = MED_IN_MAX;
			for (size_t c = 0; c < K; ++c) {
				const int32_t v = q[o * N + (size_t)r.medoid[c]];
				if (v < d) d = v, r.label[o] = (int32_t)c;
			}
			r.dist[o] = d;
		}
		++r.size[(size_t)r.label[o]], r.td += r.dist[o];
	}
	for (size_t o = 0; o < N; ++o)
		for (size_t p = 0; p < N; ++p) r.sums[o * K + (size_t)r.label[p]] += q[o * N + p];
}

double t_medoids = 0; // seconds of the k-medoids runs of the last command

// q[n][n] -> r; 0 or a PGA_ERR_* code (the table of include/pangene_hip.h pga_pan_medoids)
int medoids_run(const int32_t *q, int32_t n, int32_t k, int32_t max_iter, Medoids &r)
{
	if (q == nullptr || n < 3 || k < 2 || k > n - 1 || max_iter < 0) return PGA_ERR_ARG;
	if (n > 65535 || k > MED_MAX_K) return PGA_ERR_RANGE;
	const size_t N = (size_t)n;
	if (const int bad = fixed_matrix_ok(q, n)) return bad;
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	if (be->pan_medoids != nullptr) {
		const pga_medoids_in_t in{q, n, k, max_iter};
		pga_medoids_out_t res{};
		const int rc = be->pan_medoids(&in, &res);
		if (rc != 0) return rc;
		const size_t K = (size_t)k;
		r.medoid.assign(res.medoid, res.medoid + K), r.label.assign(res.label, res.label + N), r.dist.assign(res.dist, res.dist + N), r.size.assign(res.size, res.size + K);
		r.sums.assign(res.sums, res.sums + N * K), r.rec.assign(res.rec, res.rec + 3 * (size_t)res.n_rec);
		r.td = res.td, r.n_swap = res.n_swap, r.converged = res.converged;
	} else medoids_host(q, n, k, max_iter, r);
	t_medoids += now_sec() - t0;
	return 0;
}

// The silhouettes from sums and size alone.  With o in cluster c: a = sums[o][c] / (size_c - 1), b = the smallest sums[o][c'] / size_c'
// over c' != c (compared by cross-multiplication, the first of equal ones), s = (b - a) / max(a, b) as ONE division of the two
// cross-products X = sums[o][c'] (size_c - 1) and Y = sums[o][c] size_c'; 0 for a cluster of one and where both are 0.
void silhouettes(const Medoids &r, std::vector<double> &sil)
{
	const size_t N = r.label.size(), K = r.size.size();
	sil.assign(N, 0.0);
	for (size_t o = 0; o < N; ++o) {
		const size_t c = (size_t)r.label[o];
		const int64_t sc = r.size[c];
		if (sc == 1) continue;
		int64_t B = 0, sb = 0;
		for (size_t e = 0; e < K; ++e) {
			if (e == c) continue;
			const int64_t v = r.sums[o * K + e], se = r.size[e];
			if (sb == 0 || v * sb < B * se) B = v, sb = se;
		}
		const int64_t X = B * (sc - 1), Y = r.sums[o * K + c] * sb, mx = std::max(X, Y);
		if (mx != 0) sil[o] = (double)(X - Y) / (double)mx;
	}
}

// the mean over the columns of cluster c (c < 0: over all of them), summed in column order
double mean_sil(const Medoids &r, const std::vector<double> &sil, int32_t c)
{
	double s = 0;
	int64_t cnt = 0;
	for (size_t o = 0; o < sil.size(); ++o)
		if (c < 0 || r.label[o] == c) s += sil[o], ++cnt;
	return s / (double)cnt;
}

std::string fixed_text(int64_t v, int32_t F)
{
	char b[64];
	std::snprintf(b, sizeof(b), "%.6f", (double)v / (double)((int64_t)1 << F));
	return b;
}

int cluster_run(const ItemSource &src, const pg_cluster_opt_t *o)
{
	const double t_start = now_sec();
	std::vector<std::string> names;
	std::vector<uint32_t> bits;
	int32_t M;
	if (src(o->type, names, bits, M) != 0) return PAN_NO_ITEMS;
	if ((o->type != PG_DIST_GENE && o->type != PG_DIST_ADJ) || (o->metric != PG_DIST_JACCARD && o->metric != PG_DIST_DIFF) || o->max_iter < 0) return PGA_ERR_ARG;
	const int32_t A = (int32_t)names.size();
	if (A < 3) { std::fprintf(stderr, "Error: pangene cluster needs at least 3 assemblies, the input has %d\n", A); return PGA_ERR_ARG; }
	if (o->k_lo < 2 || o->k_hi < o->k_lo || o->k_hi > A - 1) {
		std::fprintf(stderr, "Error: pangene cluster: k must be in [2, %d] for %d assemblies\n", A - 1, A);
		return PGA_ERR_ARG;
	}
	const double t_prep = now_sec() - t_start;
	std::vector<int32_t> q;
	int32_t F = 20;
	int rc = fixed_dist(bits, M, A, o->metric, q, &F);
	if (rc != 0) return rc;
	t_medoids = 0;
	OutBuf ob;
	std::string &s = ob.s;
	char b[128];
	s = "#K\tk\tTD\tmean_sil\tswaps\tconverged\n";
	Medoids best, cur;
	std::vector<double> best_sil, sil;
	double best_mean = 0;
	for (int32_t k = o->k_lo; k <= o->k_hi; ++k) {
		if ((rc = medoids_run(q.data(), A, k, o->max_iter, cur)) != 0) return rc;
		if (!cur.converged) std::fprintf(stderr, "Note: pangene cluster: k = %d did not converge within %d iterations\n", k, o->max_iter);
		silhouettes(cur, sil);
		const double mean = mean_sil(cur, sil, -1);
		std::snprintf(b, sizeof(b), "\t%.4f\t%d\t%d\n", mean, cur.n_swap, cur.converged);
		s += "K\t" + std::to_string(k) + "\t" + fixed_text(cur.td, F) + b;
		if (k == o->k_lo || mean > best_mean) best_mean = mean, std::swap(best, cur), std::swap(best_sil, sil);
	}
	const double t1 = now_sec();
	s += "#C\tcluster\tmedoid\tsize\tmean_sil\n";
	for (size_t c = 0; c < best.medoid.size(); ++c) {
		std::snprintf(b, sizeof(b), "\t%d\t%.4f\n", best.size[c], mean_sil(best, best_sil, (int32_t)c));
		s += "C\t" + std::to_string(c + 1) + "\t" + names[(size_t)best.medoid[c]] + b;
	}
	s += "#A\tassembly\tcluster\tmedoid\tdist\tsil\n";
	for (size_t x = 0; x < (size_t)A; ++x) {
		const size_t c = (size_t)best.label[x];
		std::snprintf(b, sizeof(b), "\t%.4f\n", best_sil[x]);
		s += "A\t" + names[x] + "\t" + std::to_string(c + 1) + "\t" + names[(size_t)best.medoid[c]] + "\t" + fixed_text(best.dist[x], F) + b;
		ob.flush_if_full();
	}
	ob.finish();
	if (std::getenv("PANGENE_CLUSTER_TIMING") != nullptr)
		std::fprintf(stderr, "[cluster-timing] route=%s items=%d assemblies=%d prep_ms=%.3f medoids_ms=%.3f write_ms=%.3f\n", src.route(), M, A, t_prep * 1e3, t_medoids * 1e3,
		             (now_sec() - t1) * 1e3);
	return 0;
}

// a run's results into the caller's arrays; rec takes the first rec_cap records
void medoids_copy(const Medoids &r, int32_t *medoid, int32_t *label, int32_t *dist, int32_t *size, int64_t *sums, int64_t *rec, int32_t rec_cap, int32_t *n_rec,
                  int32_t *n_swap, int64_t *td, int32_t *converged)
{
	std::copy(r.medoid.begin(), r.medoid.end(), medoid), std::copy(r.label.begin(), r.label.end(), label), std::copy(r.dist.begin(), r.dist.end(), dist);
	std::copy(r.size.begin(), r.size.end(), size), std::copy(r.sums.begin(), r.sums.end(), sums);
	const size_t nr = r.rec.size() / 3;
	std::copy(r.rec.begin(), r.rec.begin() + (std::ptrdiff_t)(3 * std::min(nr, (size_t)std::max(rec_cap, 0))), rec);
	*n_rec = (int32_t)nr, *n_swap = r.n_swap, *td = r.td, *converged = r.converged;
}

} // namespace
} // namespace pgx

extern "C" {

void pg_cluster_opt_init(pg_cluster_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->k_lo = o->k_hi = 2, o->max_iter = 1000;
}

int pg_cluster_file(const char *gfa_fn, const pg_cluster_opt_t *o) { return file_result(cluster_run(items_of_file(gfa_fn), o), gfa_fn, "pangene cluster"); }
void pg_write_cluster(pg_graph_t *q, const pg_cluster_opt_t *o) { graph_result(cluster_run(items_of_graph(q), o), "pg_write_cluster"); }

int pg_pan_medoids(const int32_t *q, int32_t n, int32_t k, int32_t max_iter, int32_t *medoid, int32_t *label, int32_t *dist, int32_t *size, int64_t *sums, int64_t *rec,
                   int32_t rec_cap, int32_t *n_rec, int32_t *n_swap, int64_t *td, int32_t *converged)
{
	if (medoid == nullptr || label == nullptr || dist == nullptr || size == nullptr || sums == nullptr || (rec == nullptr && rec_cap > 0) || n_rec == nullptr ||
	    n_swap == nullptr || td == nullptr || converged == nullptr) return PGA_ERR_ARG;
	Medoids r;
	const int rc = medoids_run(q, n, k, max_iter, r);
	if (rc == 0) medoids_copy(r, medoid, label, dist, size, sums, rec, rec_cap, n_rec, n_swap, td, converged);
	return rc;
}

int pg_pan_cluster(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, int32_t k, int32_t max_iter, int32_t *medoid, int32_t *label, int32_t *dist,
                   int32_t *size, int64_t *sums, int64_t *rec, int32_t rec_cap, int32_t *n_rec, int32_t *n_swap, int64_t *td, int32_t *converged, int32_t *frac_bits)
{
	if ((metric != PG_DIST_JACCARD && metric != PG_DIST_DIFF) || n_item < 0 || n_asm < 3 || ((size_t)n_item > 0 && presence == nullptr) || frac_bits == nullptr) return PGA_ERR_ARG;
	if (medoid == nullptr || label == nullptr || dist == nullptr || size == nullptr || sums == nullptr || (rec == nullptr && rec_cap > 0) || n_rec == nullptr ||
	    n_swap == nullptr || td == nullptr || converged == nullptr) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	std::vector<int32_t> q;
	int rc = fixed_dist(bits, n_item, n_asm, metric, q, frac_bits);
	if (rc != 0) return rc;
	Medoids r;
	if ((rc = medoids_run(q.data(), n_asm, k, max_iter, r)) == 0) medoids_copy(r, medoid, label, dist, size, sums, rec, rec_cap, n_rec, n_swap, td, converged);
	return rc;
}

} // extern "C"
