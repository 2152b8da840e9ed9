// dist.cpp -- pairwise distances of the assemblies (pg_dist_file, pg_write_dist, pg_pan_shared, pg_pan_dist; include/pangene_amd.h).
// Each assembly is a bit set over items -- its genes (the gfa2matrix matrix) or the gene adjacencies its walks traverse -- and every
// metric is arithmetic on S[i][j] = |B_i & B_j|.  S is counted on the backend (pga_pan_shared), or by the plain loops below when the
// backend has no such entry.
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>
#include "pg_internal.hpp"

namespace pgx {
int walk_lists(pg_graph_t *q, std::vector<std::string> &asm_name, std::vector<int32_t> &step, std::vector<int64_t> &walk_off); // gfa_writer.cpp

namespace {

// The backend's step on the host: S[i][j] for j >= i, mirrored.  bits[A][W]
void shared_host(const uint32_t *bits, int32_t A, int32_t W, int32_t *S)
{
	for (int32_t i = 0; i < A; ++i) {
		const uint32_t *bi = bits + (size_t)i * W;
		for (int32_t j = i; j < A; ++j) {
			const uint32_t *bj = bits + (size_t)j * W;
			int32_t s = 0;
			for (int32_t k = 0; k < W; ++k) s += __builtin_popcount(bi[k] & bj[k]);
			S[(size_t)i * A + j] = S[(size_t)j * A + i] = s;
		}
	}
}

double t_count = 0; // seconds of the last count step (backend or host loops)

} // namespace

// bits[A][(M + 31) / 32] -> S[A][A]; 0 or a PGA_ERR_* code
int shared_count(const std::vector<uint32_t> &bits, int32_t M, int32_t A, int32_t *S)
{
	if (M < 0 || A < 0) return PGA_ERR_ARG;
	const int32_t W = (int32_t)(((int64_t)M + 31) / 32);
	const size_t nn = (size_t)A * (size_t)A;
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	if (be->pan_shared != nullptr) {
		const pga_shared_in_t in{bits.data(), M, A};
		pga_shared_out_t res{};
		const int rc = be->pan_shared(&in, &res);
		if (rc != 0) return rc;
		if (nn) std::memcpy(S, res.shared, sizeof(int32_t) * nn);
	} else shared_host(bits.data(), A, W, S);
	t_count = now_sec() - t0;
	return 0;
}

namespace {

// walks (steps = segment * 2 + reverse; walk w of assembly walk_asm[w]) -> the adjacencies of each assembly as bit rows; M = the
// distinct adjacencies.  (u, v) and (v ^ 1, u ^ 1) are the same adjacency read from the other strand; the smaller pair is the key.
// key_of: nullptr, or receives the key u << 32 | v of every adjacency
void adj_bits(const std::vector<int32_t> &step, const std::vector<int64_t> &walk_off, const std::vector<int32_t> &walk_asm, int32_t A,
              std::vector<uint32_t> &bits, int32_t &M, std::vector<uint64_t> *key_of = nullptr)
{
	std::unordered_map<uint64_t, int32_t> id;
	std::vector<std::pair<int32_t, int32_t>> has; // (assembly, item)
	for (size_t w = 0; w + 1 < walk_off.size(); ++w)
		for (int64_t k = walk_off[w] + 1; k < walk_off[w + 1]; ++k) {
			const uint32_t u = (uint32_t)step[(size_t)k - 1], v = (uint32_t)step[(size_t)k];
			const uint64_t f = (uint64_t)u << 32 | v, r = (uint64_t)(v ^ 1u) << 32 | (u ^ 1u);
			auto it = id.emplace(f < r ? f : r, (int32_t)id.size()).first;
			has.emplace_back(walk_asm[w], it->second);
		}
	M = (int32_t)id.size();
	if (key_of != nullptr) {
		key_of->resize(id.size());
		for (const auto &kv : id) (*key_of)[(size_t)kv.second] = kv.first;
	}
	const size_t W = ((size_t)M + 31) / 32;
	bits.assign((size_t)A * W, 0);
	for (const auto &h : has) bits[(size_t)h.first * W + (size_t)(h.second >> 5)] |= 1u << (h.second & 31);
}

// what an item is called: a gene by its name, an adjacency by its two steps as a walk writes them (>a<b)
void adj_names(const std::vector<uint64_t> &key, const std::vector<std::string> &seg, std::vector<std::string> &item_names)
{
	item_names.clear();
	item_names.reserve(key.size());
	for (const uint64_t k : key) {
		const uint32_t u = (uint32_t)(k >> 32), v = (uint32_t)k;
		item_names.push_back((u & 1u ? "<" : ">") + seg[u >> 1] + (v & 1u ? "<" : ">") + seg[v >> 1]);
	}
}

} // namespace

// the items of the assemblies of a GFA file as bit rows (0, or -1 when the file cannot be opened), and of the graph in memory;
// item_names: nullptr, or receives what each item is called
int dist_items_file(const char *gfa_fn, int32_t type, std::vector<std::string> &names, std::vector<uint32_t> &bits, int32_t &M, std::vector<std::string> *item_names)
{
	GfaMatrix m;
	if (gfa_matrix(gfa_fn, m) != 0) return -1;
	const int32_t A = (int32_t)m.asm_a.size();
	if (type == PG_DIST_ADJ) {
		std::vector<uint64_t> key;
		adj_bits(m.step, m.walk_off, m.walk_asm, A, bits, M, item_names ? &key : nullptr);
		if (item_names) adj_names(key, m.seg, *item_names);
	} else {
		M = (int32_t)m.seg.size(), pack_cols(m.mat.data(), M, A, bits); // gene g is in assembly a when its entry is > 0
		if (item_names) item_names->swap(m.seg);
	}
	names.swap(m.asm_a);
	return 0;
}

int dist_items_graph(pg_graph_t *q, int32_t type, std::vector<std::string> &names, std::vector<uint32_t> &bits, int32_t &M, std::vector<std::string> *item_names)
{
	names.clear();
	std::vector<std::string> seg;
	if (item_names) {
		seg.reserve((size_t)q->n_seg);
		for (int32_t i = 0; i < q->n_seg; ++i) seg.emplace_back(q->d->gene[q->seg[i].gid].name);
	}
	if (type == PG_DIST_ADJ) {
		// the walks pg_write_walk prints; the columns are their sample#hap in first-seen order, as gfa2matrix reads them back
		std::vector<std::string> walk_name;
		std::vector<int32_t> step;
		std::vector<int64_t> walk_off;
		if (walk_lists(q, walk_name, step, walk_off) != 0) return -1;
		std::unordered_map<std::string, int32_t> col;
		std::vector<int32_t> walk_asm(walk_name.size());
		for (size_t w = 0; w < walk_name.size(); ++w) {
			auto it = col.emplace(walk_name[w], (int32_t)names.size());
			if (it.second) names.push_back(walk_name[w]);
			walk_asm[w] = it.first->second;
		}
		std::vector<uint64_t> key;
		adj_bits(step, walk_off, walk_asm, (int32_t)names.size(), bits, M, item_names ? &key : nullptr);
		if (item_names) adj_names(key, seg, *item_names);
	} else {
		std::vector<int32_t> mat;
		if (graph_matrix(q, names, mat) != 0) return -1;
		M = q->n_seg;
		pack_cols(mat.data(), M, (int32_t)names.size(), bits);
		if (item_names) item_names->swap(seg);
	}
	return 0;
}

namespace {

double metric_of(int32_t metric, int32_t ni, int32_t nj, int32_t s)
{
	if (metric == PG_DIST_SHARED) return s;
	if (metric == PG_DIST_DIFF) return (double)ni + (double)nj - 2.0 * (double)s;
	const int64_t u = (int64_t)ni + nj - s;
	return u == 0 ? 0.0 : 1.0 - (double)s / (double)u;
}

void print_dist(const std::vector<std::string> &names, const std::vector<int32_t> &S, const pg_dist_opt_t *o)
{
	const int32_t A = (int32_t)names.size();
	OutBuf ob;
	std::string &s = ob.s;
	if (o->phylip) s = std::to_string(A), s += '\n';
	else {
		s = "Asm";
		for (const std::string &n : names) s += '\t', s += n;
		s += '\n';
	}
	char b[40];
	for (int32_t i = 0; i < A; ++i) {
		s += names[(size_t)i];
		const int32_t ni = S[(size_t)i * A + i];
		for (int32_t j = 0; j < A; ++j) {
			const int32_t nj = S[(size_t)j * A + j], x = S[(size_t)i * A + j];
			if (o->metric == PG_DIST_JACCARD) std::snprintf(b, sizeof(b), "\t%.6f", metric_of(PG_DIST_JACCARD, ni, nj, x));
			else std::snprintf(b, sizeof(b), "\t%lld", (long long)metric_of(o->metric, ni, nj, x));
			s += b;
		}
		s += '\n';
		ob.flush_if_full();
	}
	ob.finish();
}

// PANGENE_DIST_TIMING=1: one line on stderr per call
void report_time(const char *route, int32_t M, int32_t A, double t_prep, double t_write)
{
	if (std::getenv("PANGENE_DIST_TIMING") == nullptr) return;
	std::fprintf(stderr, "[dist-timing] route=%s items=%d assemblies=%d prep_ms=%.3f count_ms=%.3f write_ms=%.3f\n", route, M, A,
	             t_prep * 1e3, t_count * 1e3, t_write * 1e3);
}

int dist_run(const char *route, const std::vector<std::string> &names, const std::vector<uint32_t> &bits, int32_t M, const pg_dist_opt_t *o,
             double t_start)
{
	std::vector<int32_t> S(names.size() * names.size());
	const double t_prep = now_sec() - t_start;
	const int rc = shared_count(bits, M, (int32_t)names.size(), S.data());
	if (rc != 0) return rc;
	const double t1 = now_sec();
	print_dist(names, S, o);
	report_time(route, M, (int32_t)names.size(), t_prep, now_sec() - t1);
	return 0;
}

} // namespace
} // namespace pgx

using namespace pgx;

extern "C" {

void pg_dist_opt_init(pg_dist_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->phylip = 0;
}

int pg_dist_file(const char *gfa_fn, const pg_dist_opt_t *o)
{
	const double t0 = now_sec();
	std::vector<std::string> names;
	std::vector<uint32_t> bits;
	int32_t M;
	if (dist_items_file(gfa_fn, o->type, names, bits, M) != 0) return cannot_open(gfa_fn);
	const int rc = dist_run("file", names, bits, M, o, t0);
	if (rc != 0) { std::fprintf(stderr, "Error: pan_shared: %s\n", backend_default()->strerror(rc)); return -2; }
	return 0;
}

void pg_write_dist(pg_graph_t *q, const pg_dist_opt_t *o)
{
	const double t0 = now_sec();
	std::vector<std::string> names;
	std::vector<uint32_t> bits;
	int32_t M;
	if (dist_items_graph(q, o->type, names, bits, M) != 0) return;
	const int rc = dist_run("memory", names, bits, M, o, t0);
	if (rc != 0) set_error(rc, "pg_write_dist");
}

int pg_pan_shared(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t *shared)
{
	if (n_item < 0 || n_asm < 0 || ((size_t)n_item * (size_t)n_asm > 0 && presence == nullptr) || (n_asm > 0 && shared == nullptr)) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	return shared_count(bits, n_item, n_asm, shared);
}

int pg_pan_dist(const uint8_t *presence, int32_t n_item, int32_t n_asm, int32_t metric, double *out)
{
	if (metric < PG_DIST_JACCARD || metric > PG_DIST_DIFF) return PGA_ERR_ARG;
	if (n_item < 0 || n_asm < 0 || ((size_t)n_item * (size_t)n_asm > 0 && presence == nullptr) || (n_asm > 0 && out == nullptr)) return PGA_ERR_ARG;
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	const size_t A = (size_t)n_asm;
	std::vector<int32_t> S(A * A);
	const int rc = shared_count(bits, n_item, n_asm, S.data());
	if (rc != 0) return rc;
	for (size_t i = 0; i < A; ++i)
		for (size_t j = 0; j < A; ++j) out[i * A + j] = metric_of(metric, S[i * A + i], S[j * A + j], S[i * A + j]);
	return 0;
}

} // extern "C"
