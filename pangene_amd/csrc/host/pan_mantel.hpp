// pan_mantel.hpp -- Mantel test (pg_mantel_file, pg_write_mantel, pg_pan_mantel, pangene mantel; DESIGN.md section 8 "Mantel test"): two
// fixed-point matrices over the same assemblies -- two of the distances of pan_tree.hpp, or one of them and a matrix read from a file --,
// their shifts and sums, and Z of the identity order and the two permutation counts from the backend (pga_pan_mantel) or from the plain
// loops below; r, the p values and the text are code both builds share.

namespace pgx {
namespace {

constexpr int32_t MANTEL_MAX_COL = 16384, MANTEL_MAX_PERM = 2147483646; // the backend's limits (include/pangene_hip.h pga_pan_mantel)

// what one pair of matrices leaves.  skip: 0 = tested, 1 = N < 3, 2 = a constant matrix (va = 0 or vb = 0)
struct Mantel { int32_t N = 0, sx = 0, sy = 0, skip = 1; int64_t Sa = 0, Sb = 0, Saa = 0, Sbb = 0, Z = 0, n_ge = 0, n_le = 0; };

// The backend's step on the host, by the definition: Z of an order as a double loop over i < j, doubled; the identity first, then every
// permutation's order from fisher_yates_order.  a[N][N], b[N][N]
void mantel_host(const int32_t *a, const int32_t *b, int32_t N, int32_t n, uint32_t seed, Mantel &r)
{
	const size_t n_ = (size_t)N;
	std::vector<int32_t> o(n_);
	auto Z = [&]() {
		uint64_t z = 0;
		for (size_t i = 0; i < n_; ++i)
			for (size_t j = i + 1; j < n_; ++j) z += (uint64_t)a[i * n_ + j] * (uint64_t)b[(size_t)o[i] * n_ + (size_t)o[j]];
		return (int64_t)(2 * z); // both orders of the pair
	};
	for (int32_t i = 0; i < N; ++i) o[(size_t)i] = i;
	r.Z = Z();
	r.n_ge = r.n_le = 0;
	for (int32_t p = 1; p <= n; ++p) {
		fisher_yates_order(N, seed, (uint32_t)p, o.data());
		const int64_t zp = Z();
		r.n_ge += zp >= r.Z, r.n_le += zp <= r.Z;
	}
}

double t_mantel = 0; // seconds of the backend step (or the host loops) of the last command

// qx[N][N] against qy[N][N], both checked (symmetric, zero diagonal, entries in [0, 2^29)); 0 or a PGA_ERR_* code
int mantel_core(const int32_t *qx, const int32_t *qy, int32_t N, int32_t n_perm, uint32_t seed, Mantel &r)
{
	r = Mantel();
	r.N = N;
	if (N > MANTEL_MAX_COL) return PGA_ERR_RANGE;
	const size_t n_ = (size_t)N, nn = n_ * n_;
	int32_t mx = 0, my = 0;
	for (size_t k = 0; k < nn; ++k) mx = std::max(mx, qx[k]), my = std::max(my, qy[k]);
	r.sx = shift_of(mx, N), r.sy = shift_of(my, N);
	std::vector<int32_t> a(nn), b(nn);
	for (size_t k = 0; k < nn; ++k) { // (the diagonal is zero)
		const int64_t x = a[k] = qx[k] >> r.sx, y = b[k] = qy[k] >> r.sy;
		r.Sa += x, r.Sb += y, r.Saa += x * x, r.Sbb += y * y;
	}
	if (N < 3) return 0;
	const i128 M = (i128)N * (N - 1);
	if (M * r.Saa - (i128)r.Sa * r.Sa == 0 || M * r.Sbb - (i128)r.Sb * r.Sb == 0) { r.skip = 2; return 0; }
	r.skip = 0;
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	int rc = 0;
	if (be->pan_mantel != nullptr) {
		const pga_mantel_in_t in{a.data(), b.data(), N, mx >> r.sx, my >> r.sy, n_perm, seed, nullptr, nullptr};
		pga_mantel_out_t res{};
		if ((rc = be->pan_mantel(&in, &res)) == 0) r.Z = res.z, r.n_ge = res.n_ge, r.n_le = res.n_le;
	} else mantel_host(a.data(), b.data(), N, n_perm, seed, r);
	t_mantel += now_sec() - t0;
	return rc;
}

bool mantel_opt_ok(const pg_mantel_opt_t *o)
{
	auto type_ok = [](int32_t t) { return t == PG_DIST_GENE || t == PG_DIST_ADJ; };
	auto metric_ok = [](int32_t m) { return m == PG_DIST_JACCARD || m == PG_DIST_DIFF; };
	return o != nullptr && type_ok(o->x_type) && type_ok(o->y_type) && metric_ok(o->x_metric) && metric_ok(o->y_metric) && o->n_perm >= 0 && o->n_perm <= MANTEL_MAX_PERM;
}

// one side of the test: a fixed-point matrix q[names][names] and what the X / Y column prints for it
struct MantelSide { std::string label; std::vector<std::string> names; std::vector<int32_t> q; };

void blank_fields(const std::string &l, std::vector<std::string> &f) // the fields of a line between blanks and tabs
{
	f.clear();
	for (size_t i = 0; i < l.size();) {
		while (i < l.size() && (l[i] == ' ' || l[i] == '\t' || l[i] == '\r')) ++i;
		size_t e = i;
		while (e < l.size() && l[e] != ' ' && l[e] != '\t' && l[e] != '\r') ++e;
		if (e > i) f.emplace_back(l, i, e - i);
		i = e;
	}
}

// An external matrix in either form pangene dist prints: the table ("Asm" and the names, then a name and its values per line) or relaxed
// PHYLIP (a count, then a name and its values per line).  Values by strtod; q = floor(v 2^F + 0.5) with the largest F in [0, 20] that
// keeps every entry below 2^29.  0, or -1 after one line on stderr that names the file and the line
int read_matrix_file(const char *fn, MantelSide &s)
{
	std::vector<std::string> lines, f;
	if (fn == nullptr || read_lines(fn, lines) != 0) { std::fprintf(stderr, "Error: cannot open matrix file %s\n", fn ? fn : "(null)"); return -1; }
	size_t ln = 0;
	for (; ln < lines.size(); ++ln) { blank_fields(lines[ln], f); if (!f.empty()) break; }
	if (ln == lines.size()) { std::fprintf(stderr, "Error: %s: line 1: no header line\n", fn); return -1; }
	const bool table = f[0] == "Asm";
	size_t n = 0;
	s.names.clear();
	if (table) s.names.assign(f.begin() + 1, f.end()), n = s.names.size();
	else {
		const bool digits = f.size() == 1 && f[0].size() <= 9 && f[0].find_first_not_of("0123456789") == std::string::npos;
		if (!digits) { std::fprintf(stderr, "Error: %s: line %zu: neither an Asm header line nor a count\n", fn, ln + 1); return -1; }
		n = (size_t)std::strtoul(f[0].c_str(), nullptr, 10);
	}
	std::vector<double> v;
	std::vector<size_t> row_line;
	double vmax = 0;
	size_t last = ln + 1;
	for (++ln; ln < lines.size(); ++ln) {
		blank_fields(lines[ln], f);
		if (f.empty()) continue;
		const size_t row = row_line.size();
		last = ln + 1;
		if (row == n) { std::fprintf(stderr, "Error: %s: line %zu: the matrix is not square: more than %zu rows\n", fn, ln + 1, n); return -1; }
		if (f.size() != n + 1) { std::fprintf(stderr, "Error: %s: line %zu: the matrix is not square: %zu values in a row, %zu columns\n", fn, ln + 1, f.size() - 1, n); return -1; }
		if (!table) s.names.push_back(f[0]);
		else if (f[0] != s.names[row]) { std::fprintf(stderr, "Error: %s: line %zu: row %s where the header has %s\n", fn, ln + 1, f[0].c_str(), s.names[row].c_str()); return -1; }
		for (size_t j = 0; j < n; ++j) {
			char *end = nullptr;
			const double x = std::strtod(f[j + 1].c_str(), &end);
			if (end == f[j + 1].c_str() || *end != 0 || !std::isfinite(x) || !(x >= 0)) {
				std::fprintf(stderr, "Error: %s: line %zu: value %s is not a finite number >= 0\n", fn, ln + 1, f[j + 1].c_str());
				return -1;
			}
			if (j == row && x != 0) { std::fprintf(stderr, "Error: %s: line %zu: the diagonal value %s is not 0\n", fn, ln + 1, f[j + 1].c_str()); return -1; }
			v.push_back(x), vmax = std::max(vmax, x);
		}
		row_line.push_back(ln + 1);
	}
	if (row_line.size() != n) { std::fprintf(stderr, "Error: %s: line %zu: the matrix is not square: %zu rows, %zu columns\n", fn, last, row_line.size(), n); return -1; }
	std::unordered_map<std::string, size_t> at;
	for (size_t i = 0; i < n; ++i)
		if (!at.emplace(s.names[i], i).second) { std::fprintf(stderr, "Error: %s: line %zu: assembly %s is named twice\n", fn, table ? 1 : row_line[i], s.names[i].c_str()); return -1; }
	int F = 20;
	while (F >= 0 && !(std::floor(std::ldexp(vmax, F) + 0.5) < 536870912.0)) --F;
	if (F < 0) { std::fprintf(stderr, "Error: %s: the largest value %g does not fit 29 bits\n", fn, vmax); return -1; }
	s.q.resize(n * n);
	for (size_t k = 0; k < n * n; ++k) s.q[k] = (int32_t)std::floor(std::ldexp(v[k], F) + 0.5);
	for (size_t i = 0; i < n; ++i)
		for (size_t j = 0; j < i; ++j)
			if (s.q[i * n + j] != s.q[j * n + i]) {
				std::fprintf(stderr, "Error: %s: line %zu: the matrix is not symmetric: %s to %s and back differ\n", fn, row_line[i], s.names[i].c_str(), s.names[j].c_str());
				return -1;
			}
	s.label = "file";
	return 0;
}

const char *mantel_spec(int32_t type, int32_t metric)
{
	return type == PG_DIST_GENE ? (metric == PG_DIST_JACCARD ? "gene:jaccard" : "gene:diff") : (metric == PG_DIST_JACCARD ? "adj:jaccard" : "adj:diff");
}

// one side from the source's items of `type`: 0, PAN_NO_ITEMS or a PGA_ERR_* code
int mantel_side(const ItemSource &src, int32_t type, int32_t metric, MantelSide &s)
{
	std::vector<uint32_t> bits;
	int32_t M = 0, F = 20;
	if (src(type, s.names, bits, M) != 0) return PAN_NO_ITEMS;
	s.label = mantel_spec(type, metric);
	return fixed_dist(bits, M, (int32_t)s.names.size(), metric, s.q, &F);
}

// the assemblies both sides name, in X's order; a name on one side only gets a note and is left out.  Then the test and the text
int mantel_write(const ItemSource &src, const MantelSide &X, const MantelSide &Y, const pg_mantel_opt_t *o, double t_start)
{
	const double t_prep = now_sec() - t_start;
	std::unordered_map<std::string, size_t> at;
	for (size_t k = 0; k < Y.names.size(); ++k) at.emplace(Y.names[k], k);
	std::vector<size_t> ix, iy;
	std::vector<uint8_t> used(Y.names.size(), 0);
	for (size_t i = 0; i < X.names.size(); ++i) {
		const auto it = at.find(X.names[i]);
		if (it == at.end()) { std::fprintf(stderr, "Note: assembly %s is in %s only; left out\n", X.names[i].c_str(), X.label.c_str()); continue; }
		ix.push_back(i), iy.push_back(it->second), used[it->second] = 1;
	}
	for (size_t k = 0; k < Y.names.size(); ++k)
		if (!used[k]) std::fprintf(stderr, "Note: assembly %s is in %s only; left out\n", Y.names[k].c_str(), Y.label.c_str());
	const size_t n_ = ix.size(), nx = X.names.size(), ny = Y.names.size();
	std::vector<int32_t> qx(n_ * n_), qy(n_ * n_);
	for (size_t i = 0; i < n_; ++i)
		for (size_t j = 0; j < n_; ++j) qx[i * n_ + j] = X.q[ix[i] * nx + ix[j]], qy[i * n_ + j] = Y.q[iy[i] * ny + iy[j]];
	t_mantel = 0;
	Mantel r;
	const int rc = mantel_core(qx.data(), qy.data(), (int32_t)n_, o->n_perm, o->seed, r);
	if (rc != 0) return rc;
	OutBuf ob;
	std::string &s = ob.s;
	s = "X\tY\tN\tr\tn_ge\tn_le\tp_greater\tp_less\n";
	if (r.skip) std::fprintf(stderr, "Note: %s over the %d assemblies; not tested\n", r.skip == 2 ? "a matrix has one value only" : "fewer than 3 assemblies", r.N);
	else {
		const i128 M = (i128)r.N * (r.N - 1), num = M * r.Z - (i128)r.Sa * r.Sb, va = M * r.Saa - (i128)r.Sa * r.Sa, vb = M * r.Sbb - (i128)r.Sb * r.Sb;
		const long double rho = ((long double)num / sqrtl((long double)va)) / sqrtl((long double)vb);
		char b[256];
		std::snprintf(b, sizeof(b), "\t%d\t%.4Lf\t%lld\t%lld\t", r.N, rho, (long long)r.n_ge, (long long)r.n_le);
		s += X.label, s += '\t', s += Y.label, s += b;
		if (o->n_perm > 0) std::snprintf(b, sizeof(b), "%.6f\t%.6f\n", ((double)r.n_ge + 1.0) / ((double)o->n_perm + 1.0), ((double)r.n_le + 1.0) / ((double)o->n_perm + 1.0));
		else std::snprintf(b, sizeof(b), "NA\tNA\n");
		s += b;
	}
	ob.finish();
	if (std::getenv("PANGENE_MANTEL_TIMING") != nullptr)
		std::fprintf(stderr, "[mantel-timing] route=%s assemblies=%d perms=%d prep_ms=%.3f stat_ms=%.3f all_ms=%.3f\n", src.route(), r.N, o->n_perm, t_prep * 1e3,
		             t_mantel * 1e3, (now_sec() - t_start) * 1e3);
	return 0;
}

// both sides, then mantel_write
int mantel_run(const ItemSource &src, const char *mat_fn, const pg_mantel_opt_t *o)
{
	const double t_start = now_sec();
	if (!mantel_opt_ok(o)) return PGA_ERR_ARG;
	MantelSide X, Y;
	int rc = mantel_side(src, o->x_type, o->x_metric, X);
	if (rc != 0) return rc;
	if (mat_fn != nullptr) { if (read_matrix_file(mat_fn, Y) != 0) return PAN_BAD_FILE; }
	else if ((rc = mantel_side(src, o->y_type, o->y_metric, Y)) != 0) return rc;
	return mantel_write(src, X, Y, o, t_start);
}

} // namespace
} // namespace pgx

extern "C" {

void pg_mantel_opt_init(pg_mantel_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->x_type = PG_DIST_GENE, o->x_metric = PG_DIST_JACCARD, o->y_type = PG_DIST_ADJ, o->y_metric = PG_DIST_JACCARD, o->n_perm = 1000, o->seed = 11;
}

int pg_mantel_file(const char *gfa_fn, const char *mat_fn, const pg_mantel_opt_t *o)
{
	if (o == nullptr) { std::fprintf(stderr, "Error: pan_mantel: no options\n"); return -2; }
	return file_result(mantel_run(items_of_file(gfa_fn), mat_fn, o), gfa_fn, "pan_mantel");
}

void pg_write_mantel(pg_graph_t *q, const char *mat_fn, const pg_mantel_opt_t *o)
{
	if (o == nullptr) { set_error(PGA_ERR_ARG, "pg_write_mantel"); return; }
	graph_result(mantel_run(items_of_graph(q), mat_fn, o), "pg_write_mantel", "pg_write_mantel: bad matrix file");
}

int pg_pan_mantel(const int32_t *qx, const int32_t *qy, int32_t n, const pg_mantel_opt_t *o, int64_t *out)
{
	if (n < 0 || !mantel_opt_ok(o) || out == nullptr || (n > 0 && (qx == nullptr || qy == nullptr))) return PGA_ERR_ARG;
	if (n > MANTEL_MAX_COL) return PGA_ERR_RANGE; // (before the matrices are looked at)
	int rc = fixed_matrix_ok(qx, n);
	if (rc == 0) rc = fixed_matrix_ok(qy, n);
	if (rc != 0) return rc;
	Mantel r;
	if ((rc = mantel_core(qx, qy, n, o->n_perm, o->seed, r)) != 0) return rc;
	out[0] = r.N, out[1] = r.sx, out[2] = r.sy, out[3] = r.Sa, out[4] = r.Sb, out[5] = r.Saa, out[6] = r.Sbb;
	out[7] = r.skip ? 0 : r.Z, out[8] = r.skip ? -1 : r.n_ge, out[9] = r.skip ? -1 : r.n_le;
	return 0;
}

} // extern "C"
