// pan_phylosig.hpp -- phylogenetic signal of the items on the tree of the assemblies (pg_phylosig_file, pg_write_phylosig,
// pg_pan_phylosig, pangene phylosig; DESIGN.md section 8 "Phylogenetic signal"): the permutation tail of the parsimony cost and the
// retention index.  Items, tree and observed costs are pangene gainloss's (pan_gainloss.hpp, included before this header).  The
// permutation step -- classes x permutations up passes, the counts per item and the sums per class -- runs on the backend
// (pga_pan_phylosig: the tree as the postfix program, the orders made on the device), or as the plain loops below over the tree records
// when the backend has no such entry; the classes, the ratios and the table are code both builds share.

namespace pgx {
namespace {

// The backend's step on the host, by the definition and over the tree itself (no program, no reordering): per class and permutation the
// order of fisher_yates_order, the tip set o[x] < n, the way up of gainloss_host.  kid as pairs_tree makes it, A >= 2; cls[n_cls]
// ascending, each in 1 .. A - 1; n_le, n_ge[n_item], sum[n_cls]
void phylosig_host(int32_t A, const std::vector<int32_t> &kid, int32_t g, int32_t l, const std::vector<int32_t> &cls, const std::vector<int32_t> &item_cls,
                   const std::vector<int32_t> &item_cost, int32_t n_perm, uint32_t seed, int32_t *n_le, int32_t *n_ge, int64_t *sum)
{
	const size_t n_node = (size_t)A + kid.size() / 2, root = n_node - 1, n_cls = cls.size(), n_item = item_cls.size();
	std::vector<int32_t> C(2 * n_node), o((size_t)A), cost(n_cls);
	std::fill(n_le, n_le + n_item, 0), std::fill(n_ge, n_ge + n_item, 0), std::fill(sum, sum + n_cls, (int64_t)0);
	for (int32_t p = 1; p <= n_perm; ++p) {
		for (size_t c = 0; c < n_cls; ++c) {
			fisher_yates_order(A, seed, (uint32_t)p, o.data());
			for (int32_t x = 0; x < A; ++x) {
				const int32_t b = o[(size_t)x] < cls[c];
				C[2 * (size_t)x + (size_t)b] = 0, C[2 * (size_t)x + (size_t)(1 - b)] = g + l;
			}
			wagner_up(kid, A, g, l, C.data());
			cost[c] = std::min(C[2 * root], C[2 * root + 1]);
			sum[c] += cost[c];
		}
		for (size_t i = 0; i < n_item; ++i) {
			const int32_t c = cost[(size_t)item_cls[i]];
			n_le[i] += c <= item_cost[i], n_ge[i] += c >= item_cost[i];
		}
	}
}

double t_phylosig = 0; // seconds of the backend step (or the host loops) of the last command

bool phylosig_cost_ok(const pg_phylosig_opt_t *o)
{
	return o != nullptr && o->gain >= 1 && o->gain <= 255 && o->loss >= 1 && o->loss <= 255 && o->n_perm >= 0 && o->n_perm <= 2147483646 && o->min_count >= 1;
}

bool phylosig_opt_ok(const pg_phylosig_opt_t *o)
{
	return phylosig_cost_ok(o) && (o->type == PG_DIST_GENE || o->type == PG_DIST_ADJ) && (o->metric == PG_DIST_JACCARD || o->metric == PG_DIST_DIFF) &&
	       (o->method == PG_TREE_NJ || o->method == PG_TREE_UPGMA) && o->max_p >= 0.0;
}

struct PhylosigResult {
	std::vector<int32_t> gene;     // [M][5] = present, cost, gains, losses, root of gainloss_core
	std::vector<int32_t> tested;   // the tested items, ascending
	std::vector<int32_t> cls;      // the classes, ascending
	std::vector<int32_t> item_cls; // [tested.size()] index into cls
	std::vector<int32_t> n_le, n_ge; // [tested.size()]
	std::vector<int64_t> sum;      // [cls.size()]
};

// bits[A][W] over M items, the tree of kid (pairs_tree), A >= 1: the observed costs, the classes, the counts and the sums.  0 or a PGA_ERR_* code
int phylosig_core(const std::vector<uint32_t> &bits, int32_t M, int32_t A, const std::vector<int32_t> &kid, const pg_phylosig_opt_t *o, PhylosigResult &r)
{
	r.gene.assign(5 * (size_t)M, 0);
	std::vector<int64_t> node(3 * ((size_t)A + kid.size() / 2));
	t_gainloss = 0;
	int rc = gainloss_core(bits, M, A, kid, o->gain, o->loss, PG_GAINLOSS_LATE, r.gene.data(), node.data());
	if (rc != 0) return rc;
	const double t0 = now_sec();
	std::vector<int32_t> slot((size_t)A + 1, -1); // class index by size
	std::vector<int32_t> item_cost;
	for (int32_t i = 0; i < M; ++i) {
		const int32_t n = r.gene[5 * (size_t)i];
		if (std::min(n, A - n) < o->min_count) continue;
		r.tested.push_back(i), item_cost.push_back(r.gene[5 * (size_t)i + 1]);
		slot[(size_t)n] = 0;
	}
	for (int32_t n = 0; n <= A; ++n)
		if (slot[(size_t)n] == 0) slot[(size_t)n] = (int32_t)r.cls.size(), r.cls.push_back(n);
	for (const int32_t i : r.tested) r.item_cls.push_back(slot[(size_t)r.gene[5 * (size_t)i]]);
	const size_t n_item = r.tested.size(), n_cls = r.cls.size();
	r.n_le.assign(n_item, 0), r.n_ge.assign(n_item, 0), r.sum.assign(n_cls, 0);
	if (n_item == 0 || o->n_perm == 0) return 0;
	const pga_backend_t *be = backend_default();
	if (be->pan_phylosig != nullptr) {
		std::vector<uint8_t> op;
		std::vector<int32_t> leaf;
		if (pairs_program(kid, A, op, leaf) > GAINLOSS_DEPTH) return PGA_ERR_RANGE; // (out of reach below 65 536 leaves)
		const pga_phylosig_in_t in{op.data(), leaf.data(), A, o->gain, o->loss, (int32_t)n_cls, r.cls.data(), (int32_t)n_item, r.item_cls.data(), item_cost.data(),
		                           o->n_perm, o->seed, nullptr, nullptr};
		pga_phylosig_out_t res{};
		if ((rc = be->pan_phylosig(&in, &res)) != 0) return rc;
		std::copy(res.n_le, res.n_le + n_item, r.n_le.begin()), std::copy(res.n_ge, res.n_ge + n_item, r.n_ge.begin()), std::copy(res.sum, res.sum + n_cls, r.sum.begin());
	} else phylosig_host(A, kid, o->gain, o->loss, r.cls, r.item_cls, item_cost, o->n_perm, o->seed, r.n_le.data(), r.n_ge.data(), r.sum.data());
	t_phylosig += now_sec() - t0;
	return 0;
}

const char *const PHYLOSIG_HEADER = "Gene\tPresent\tCost\tMaxCost\tExpect\tRI\tn_le\tn_ge\tp_signal\tp_scatter\tq_signal\n";

// the items, the tree of all assemblies, the observed costs, the permutations, the table
int phylosig_run(const ItemSource &src, const pg_phylosig_opt_t *o)
{
	const double t_start = now_sec();
	if (!phylosig_opt_ok(o)) return PGA_ERR_ARG;
	std::vector<std::string> names, item;
	std::vector<uint32_t> bits;
	int32_t M = 0;
	if (src(o->type, names, bits, M, &item) != 0) return PAN_NO_ITEMS;
	const int32_t A = (int32_t)names.size();
	const double t_prep = now_sec() - t_start;
	OutBuf ob;
	std::string &s = ob.s;
	s = PHYLOSIG_HEADER;
	if (A == 0 || M == 0) { ob.finish(); return 0; }
	if (A > GAINLOSS_MAX_LEAF || M > GAINLOSS_MAX_ITEM) return PGA_ERR_RANGE;
	const double t1 = now_sec();
	std::vector<int64_t> rec((size_t)6 * (size_t)A);
	int rc = tree_joins(bits, M, A, o->metric, o->method, rec.data());
	if (rc != 0) return rc;
	const double t_tree = now_sec() - t1;
	std::vector<int32_t> kid;
	if (!pairs_tree(rec.data(), A, o->method, kid)) return PGA_ERR_ARG;
	PhylosigResult r;
	t_phylosig = 0;
	if ((rc = phylosig_core(bits, M, A, kid, o, r)) != 0) return rc;
	const size_t n_item = r.tested.size();
	const double P = (double)o->n_perm;
	std::vector<double> ps(n_item), pc(n_item), q;
	for (size_t k = 0; k < n_item; ++k) ps[k] = (1.0 + (double)r.n_le[k]) / (1.0 + P), pc[k] = (1.0 + (double)r.n_ge[k]) / (1.0 + P);
	bh_q(ps, q);
	char b[256], ri[32];
	for (size_t k = 0; k < n_item; ++k) {
		if (o->n_perm > 0 && std::min(ps[k], pc[k]) > o->max_p) continue;
		const int32_t *gn = r.gene.data() + 5 * (size_t)r.tested[k];
		const int64_t n = gn[0], cost = gn[1], max_cost = std::min(n * o->gain, ((int64_t)A - n) * o->loss), den = max_cost - std::min(o->gain, o->loss);
		if (den == 0) std::snprintf(ri, sizeof(ri), "NA");
		else std::snprintf(ri, sizeof(ri), "%.4f", (double)(max_cost - cost) / (double)den);
		if (o->n_perm > 0)
			std::snprintf(b, sizeof(b), "\t%d\t%d\t%lld\t%.3f\t%s\t%d\t%d\t%.6f\t%.6f\t%.6f\n", gn[0], gn[1], (long long)max_cost, (double)r.sum[(size_t)r.item_cls[k]] / P, ri, r.n_le[k],
			              r.n_ge[k], ps[k], pc[k], q[k]);
		else std::snprintf(b, sizeof(b), "\t%d\t%d\t%lld\tNA\t%s\tNA\tNA\tNA\tNA\tNA\n", gn[0], gn[1], (long long)max_cost, ri);
		s += item[(size_t)r.tested[k]], s += b;
		ob.flush_if_full();
	}
	ob.finish();
	if (std::getenv("PANGENE_PHYLOSIG_TIMING") != nullptr)
		std::fprintf(stderr, "[phylosig-timing] route=%s items=%d assemblies=%d tested=%zu classes=%zu perms=%d prep_ms=%.3f tree_ms=%.3f dp_ms=%.3f perm_ms=%.3f all_ms=%.3f\n", src.route(),
		             M, A, n_item, r.cls.size(), o->n_perm, t_prep * 1e3, t_tree * 1e3, t_gainloss * 1e3, t_phylosig * 1e3, (now_sec() - t_start) * 1e3);
	return 0;
}

} // namespace
} // namespace pgx

extern "C" {

void pg_phylosig_opt_init(pg_phylosig_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->method = PG_TREE_UPGMA, o->gain = 1, o->loss = 1, o->n_perm = 1000, o->seed = 11, o->min_count = 2, o->max_p = 1.0;
}

int pg_phylosig_file(const char *gfa_fn, const pg_phylosig_opt_t *o)
{
	if (o == nullptr) { std::fprintf(stderr, "Error: pan_phylosig: no options\n"); return -2; }
	return file_result(phylosig_run(items_of_file(gfa_fn), o), gfa_fn, "pan_phylosig");
}

void pg_write_phylosig(pg_graph_t *q, const pg_phylosig_opt_t *o)
{
	if (o == nullptr) { set_error(PGA_ERR_ARG, "pg_write_phylosig"); return; }
	graph_result(phylosig_run(items_of_graph(q), o), "pg_write_phylosig");
}

int pg_pan_phylosig(const uint8_t *presence, int32_t n_item, int32_t n_asm, const int64_t *rec, int32_t method, const pg_phylosig_opt_t *o, int32_t *out_i32, int64_t *out_sum_i64)
{
	if (n_item < 0 || n_asm < 0 || (method != PG_TREE_NJ && method != PG_TREE_UPGMA) || (n_asm >= 3 && rec == nullptr) || !phylosig_cost_ok(o)) return PGA_ERR_ARG;
	if (((size_t)n_item * (size_t)n_asm > 0 && presence == nullptr) || (n_item > 0 && out_i32 == nullptr) || out_sum_i64 == nullptr) return PGA_ERR_ARG;
	if (n_asm > GAINLOSS_MAX_LEAF || n_item > GAINLOSS_MAX_ITEM) return PGA_ERR_RANGE;
	std::vector<int32_t> kid;
	if (!pairs_tree(rec, n_asm, method, kid)) return PGA_ERR_ARG;
	std::fill(out_i32, out_i32 + 5 * (size_t)n_item, 0);
	std::fill(out_sum_i64, out_sum_i64 + (size_t)n_asm + 1, (int64_t)0);
	if (n_asm == 0) return 0; // no tree: nothing is tested
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	PhylosigResult r;
	t_phylosig = 0;
	const int rc = phylosig_core(bits, n_item, n_asm, kid, o, r);
	if (rc != 0) return rc;
	for (size_t i = 0; i < (size_t)n_item; ++i) out_i32[5 * i] = r.gene[5 * i], out_i32[5 * i + 1] = r.gene[5 * i + 1];
	for (size_t k = 0; k < r.tested.size(); ++k) {
		int32_t *t = out_i32 + 5 * (size_t)r.tested[k];
		t[2] = 1, t[3] = r.n_le[k], t[4] = r.n_ge[k];
	}
	for (size_t c = 0; c < r.cls.size(); ++c) out_sum_i64[(size_t)r.cls[c]] = r.sum[c];
	return 0;
}

} // extern "C"
