// pan_gainloss.hpp -- gene gain and loss on the tree of the assemblies (pg_gainloss_file, pg_write_gainloss, pg_pan_gainloss, pangene
// gainloss; DESIGN.md section 8 "Gain and loss"): Wagner parsimony per item over the records of pangene tree.  The two passes run on the
// backend (pga_pan_gainloss: the tree as the postfix program of pan_treeprog.hpp, the items as bit rows in push order), or as the plain
// loops below over the records themselves when the backend has no such entry; the item counts, the node numbering and the two tables are
// code both builds share.

namespace pgx {
namespace {

constexpr int32_t GAINLOSS_MAX_LEAF = 65535, GAINLOSS_MAX_ITEM = 16777215, GAINLOSS_DEPTH = 16; // the backend's limits (include/pangene_hip.h pga_pan_gainloss)

inline uint32_t item_bit(const uint32_t *bits, size_t W, int32_t a, int32_t i) { return bits[(size_t)a * W + (size_t)(i >> 5)] >> (i & 31) & 1u; }

// The way up of one item or replicate: C[2 v + s] = the cheapest cost of the subtree of node v with v in state s.  The leaves' entries
// 0 .. A - 1 are set; the joins follow bottom-up in join order.  Shared with pan_phylosig.hpp.
inline void wagner_up(const std::vector<int32_t> &kid, int32_t A, int32_t g, int32_t l, int32_t *C)
{
	const int32_t w[2] = {g, l};
	for (size_t t = 0; t < kid.size() / 2; ++t)
		for (int32_t s = 0; s < 2; ++s) {
			int32_t sum = 0;
			for (int32_t c = 0; c < 2; ++c) {
				const int32_t *cc = C + 2 * (size_t)kid[2 * t + (size_t)c];
				sum += std::min(cc[s], cc[1 - s] + w[s]);
			}
			C[2 * ((size_t)A + t) + (size_t)s] = sum;
		}
}

// The backend's step on the host, by the definition and over the tree itself (no program, no reordering): per item every node's
// (C0, C1) bottom-up in join order, then the states top-down from the root, a join before its children.  bits[A][W], kid as pairs_tree
// makes it; gene[M][4] = cost, gains, losses, root; node[2 A - 1][3] in node id order.  A >= 1.  states: nullptr, or receives
// states[M][2 A - 1], the state of every node per item (pan_coevo.hpp reads the events off it)
void gainloss_host(const uint32_t *bits, int32_t M, int32_t A, const std::vector<int32_t> &kid, int32_t g, int32_t l, int32_t mode, int32_t *gene, int64_t *node,
                   uint8_t *states = nullptr)
{
	const size_t W = ((size_t)M + 31) / 32, n_join = kid.size() / 2, n_node = (size_t)A + n_join;
	std::vector<int32_t> C(2 * n_node);
	std::vector<uint8_t> state(n_node);
	const int32_t w[2] = {g, l};
	std::fill(node, node + 3 * n_node, 0);
	for (int32_t i = 0; i < M; ++i) {
		for (int32_t x = 0; x < A; ++x) {
			const uint32_t b = item_bit(bits, W, x, i);
			C[2 * (size_t)x + b] = 0, C[2 * (size_t)x + (1 - b)] = g + l;
		}
		wagner_up(kid, A, g, l, C.data());
		const size_t root = n_node - 1;
		state[root] = C[2 * root + 1] < C[2 * root];
		int32_t gains = 0, losses = 0;
		node[3 * root] += state[root];
		for (size_t t = n_join; t-- > 0;) {
			const int32_t s = state[(size_t)A + t];
			for (int32_t c = 0; c < 2; ++c) {
				const size_t v = (size_t)kid[2 * t + (size_t)c];
				const int32_t stay = C[2 * v + (size_t)s], move = C[2 * v + (size_t)(1 - s)] + w[s];
				const bool sw = mode == PG_GAINLOSS_EARLY ? move <= stay : move < stay;
				const int32_t sv = sw ? 1 - s : s;
				state[v] = (uint8_t)sv;
				node[3 * v] += sv;
				if (sw && sv) ++gains, ++node[3 * v + 1];
				if (sw && !sv) ++losses, ++node[3 * v + 2];
			}
		}
		int32_t *o = gene + 4 * (size_t)i;
		o[0] = C[2 * root + state[root]], o[1] = gains, o[2] = losses, o[3] = state[root];
		if (states != nullptr) std::copy(state.begin(), state.end(), states + (size_t)i * n_node);
	}
}

// present[i] = the assemblies that carry item i: eight byte counters a 64-bit word, emptied every 255 rows.  bits[A][W]
void item_counts(const uint32_t *bits, int32_t M, int32_t A, std::vector<int32_t> &present)
{
	static uint64_t spread[256];
	static const bool made = [] { for (int b = 0; b < 256; ++b) { uint64_t v = 0; for (int k = 0; k < 8; ++k) v |= (uint64_t)(b >> k & 1) << (8 * k); spread[b] = v; } return true; }();
	(void)made;
	const size_t W = ((size_t)M + 31) / 32;
	std::vector<uint64_t> acc(4 * W, 0);
	std::vector<int32_t> cnt(32 * W, 0);
	auto empty = [&]() {
		for (size_t k = 0; k < 4 * W; ++k) { for (int j = 0; j < 8; ++j) cnt[8 * k + (size_t)j] += (int32_t)(acc[k] >> (8 * j) & 0xff); acc[k] = 0; }
	};
	for (int32_t a = 0; a < A; ++a) {
		const uint32_t *row = bits + (size_t)a * W;
		for (size_t k = 0; k < W; ++k) {
			const uint32_t x = row[k];
			acc[4 * k] += spread[x & 0xff], acc[4 * k + 1] += spread[x >> 8 & 0xff], acc[4 * k + 2] += spread[x >> 16 & 0xff], acc[4 * k + 3] += spread[x >> 24];
		}
		if (a % 255 == 254) empty();
	}
	empty();
	present.assign(cnt.begin(), cnt.begin() + M);
}

double t_gainloss = 0; // seconds of the backend step (or the host loops) of the last command

// The tree of kid as the backend sees it: the postfix program (op, order: pairs_program), the node every op makes (node_of) and the op of
// its parent (par, -1 for the root); rows = the bit rows in push order.  Returns the stack entries the program needs.
int32_t gainloss_program(const std::vector<uint32_t> &bits, size_t W, int32_t A, const std::vector<int32_t> &kid, std::vector<uint8_t> &op, std::vector<int32_t> &node_of,
                         std::vector<int32_t> &par, std::vector<uint32_t> &rows)
{
	const size_t n_node = (size_t)A + kid.size() / 2;
	std::vector<int32_t> order;
	const int32_t need = pairs_program(kid, A, op, order);
	std::vector<int32_t> up(n_node, -1);
	for (size_t t = 0; t < kid.size() / 2; ++t) up[(size_t)kid[2 * t]] = up[(size_t)kid[2 * t + 1]] = A + (int32_t)t;
	// the node each op makes, and the op of its parent: a join's node is the parent of the two it takes
	std::vector<int32_t> op_of(n_node), made;
	node_of.resize(op.size()), par.resize(op.size());
	int32_t pushed = 0;
	for (size_t k = 0; k < op.size(); ++k) {
		int32_t v;
		if (op[k] == 0) v = order[(size_t)pushed++];
		else v = up[(size_t)made.back()], made.pop_back(), made.pop_back();
		made.push_back(v), node_of[k] = v, op_of[(size_t)v] = (int32_t)k;
	}
	for (size_t k = 0; k < op.size(); ++k) par[k] = up[(size_t)node_of[k]] < 0 ? -1 : op_of[(size_t)up[(size_t)node_of[k]]];
	rows.resize((size_t)A * W);
	for (int32_t k = 0; k < A && W > 0; ++k) std::memcpy(rows.data() + (size_t)k * W, bits.data() + (size_t)order[(size_t)k] * W, sizeof(uint32_t) * W);
	return need;
}

// bits[A][W] over M items, the tree of kid (pairs_tree): gene_out[M][5] = present, cost, gains, losses, root; node_out[2 A - 1][3] =
// present, gains, losses in node id order (leaf x = x, join t = A + t).  A >= 1.  0 or a PGA_ERR_* code
int gainloss_core(const std::vector<uint32_t> &bits, int32_t M, int32_t A, const std::vector<int32_t> &kid, int32_t g, int32_t l, int32_t mode, int32_t *gene_out,
                  int64_t *node_out)
{
	if (A > GAINLOSS_MAX_LEAF || M > GAINLOSS_MAX_ITEM) return PGA_ERR_RANGE;
	const size_t W = ((size_t)M + 31) / 32, n_node = (size_t)A + kid.size() / 2;
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	std::vector<int32_t> present;
	item_counts(bits.data(), M, A, present);
	const int32_t *gene = nullptr;
	std::vector<int32_t> gene_h;
	if (be->pan_gainloss != nullptr) {
		std::vector<uint8_t> op;
		std::vector<int32_t> node_of, par;
		std::vector<uint32_t> rows;
		if (gainloss_program(bits, W, A, kid, op, node_of, par, rows) > GAINLOSS_DEPTH) return PGA_ERR_RANGE; // (out of reach below 65 536 leaves)
		const pga_gainloss_in_t in{op.data(), rows.data(), par.data(), M, A, g, l, mode, nullptr};
		pga_gainloss_out_t res{};
		const int rc = be->pan_gainloss(&in, &res);
		if (rc != 0) return rc;
		gene = res.gene;
		for (size_t k = 0; k < op.size(); ++k) std::memcpy(node_out + 3 * (size_t)node_of[k], res.node + 3 * k, sizeof(int64_t) * 3);
	} else {
		gene_h.resize(4 * (size_t)M);
		gainloss_host(bits.data(), M, A, kid, g, l, mode, gene_h.data(), node_out);
		gene = gene_h.data();
	}
	for (size_t i = 0; i < (size_t)M; ++i) {
		int32_t *o = gene_out + 5 * i;
		o[0] = present[i], o[1] = gene[4 * i], o[2] = gene[4 * i + 1], o[3] = gene[4 * i + 2], o[4] = gene[4 * i + 3];
	}
	t_gainloss += now_sec() - t0;
	return 0;
}

bool gainloss_cost_ok(const pg_gainloss_opt_t *o)
{
	return o != nullptr && o->gain >= 1 && o->gain <= 255 && o->loss >= 1 && o->loss <= 255 && (o->mode == PG_GAINLOSS_LATE || o->mode == PG_GAINLOSS_EARLY);
}

bool gainloss_opt_ok(const pg_gainloss_opt_t *o)
{
	return gainloss_cost_ok(o) && (o->type == PG_DIST_GENE || o->type == PG_DIST_ADJ) && (o->metric == PG_DIST_JACCARD || o->metric == PG_DIST_DIFF) &&
	       (o->method == PG_TREE_NJ || o->method == PG_TREE_UPGMA) && (o->out == PG_GAINLOSS_GENE || o->out == PG_GAINLOSS_NODE) && o->min_changes >= 0;
}

// the items, the tree of all assemblies, the two passes, one of the two tables
int gainloss_run(const ItemSource &src, const pg_gainloss_opt_t *o)
{
	const double t_start = now_sec();
	if (!gainloss_opt_ok(o)) return PGA_ERR_ARG;
	std::vector<std::string> names, item;
	std::vector<uint32_t> bits;
	int32_t M = 0;
	if (src(o->type, names, bits, M, &item) != 0) return PAN_NO_ITEMS;
	const int32_t A = (int32_t)names.size();
	const double t_prep = now_sec() - t_start;
	OutBuf ob;
	std::string &s = ob.s;
	s = o->out == PG_GAINLOSS_GENE ? "Gene\tPresent\tCost\tChanges\tGains\tLosses\tRoot\n" : "Node\tChild1\tChild2\tLeaves\tPresent\tGains\tLosses\n";
	if (A == 0 || M == 0) { ob.finish(); return 0; }
	if (A > GAINLOSS_MAX_LEAF || M > GAINLOSS_MAX_ITEM) return PGA_ERR_RANGE;
	const double t1 = now_sec();
	std::vector<int64_t> rec((size_t)6 * (size_t)A);
	int rc = tree_joins(bits, M, A, o->metric, o->method, rec.data());
	if (rc != 0) return rc;
	const double t_tree = now_sec() - t1;
	std::vector<int32_t> kid;
	if (!pairs_tree(rec.data(), A, o->method, kid)) return PGA_ERR_ARG;
	const size_t n_node = (size_t)A + kid.size() / 2;
	std::vector<int32_t> gene(5 * (size_t)M);
	std::vector<int64_t> node(3 * n_node);
	t_gainloss = 0;
	if ((rc = gainloss_core(bits, M, A, kid, o->gain, o->loss, o->mode, gene.data(), node.data())) != 0) return rc;
	char b[128];
	if (o->out == PG_GAINLOSS_GENE) {
		for (size_t i = 0; i < (size_t)M; ++i) {
			const int32_t *r = gene.data() + 5 * i;
			if (r[2] + r[3] < o->min_changes) continue;
			std::snprintf(b, sizeof(b), "\t%d\t%d\t%d\t%d\t%d\t%d\n", r[0], r[1], r[2] + r[3], r[2], r[3], r[4]);
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
			const int64_t *r = node.data() + 3 * v;
			if (v + 1 == n_node) std::snprintf(b, sizeof(b), "\t%d\t%lld\tNA\tNA\n", leaves[v], (long long)r[0]);
			else std::snprintf(b, sizeof(b), "\t%d\t%lld\t%lld\t%lld\n", leaves[v], (long long)r[0], (long long)r[1], (long long)r[2]);
			s += b;
			ob.flush_if_full();
		}
	}
	ob.finish();
	if (std::getenv("PANGENE_GAINLOSS_TIMING") != nullptr)
		std::fprintf(stderr, "[gainloss-timing] route=%s items=%d assemblies=%d prep_ms=%.3f tree_ms=%.3f dp_ms=%.3f all_ms=%.3f\n", src.route(), M, A, t_prep * 1e3,
		             t_tree * 1e3, t_gainloss * 1e3, (now_sec() - t_start) * 1e3);
	return 0;
}

} // namespace
} // namespace pgx

extern "C" {

void pg_gainloss_opt_init(pg_gainloss_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->method = PG_TREE_UPGMA, o->gain = 1, o->loss = 1, o->mode = PG_GAINLOSS_LATE, o->out = PG_GAINLOSS_GENE;
}

int pg_gainloss_file(const char *gfa_fn, const pg_gainloss_opt_t *o)
{
	if (o == nullptr) { std::fprintf(stderr, "Error: pan_gainloss: no options\n"); return -2; }
	return file_result(gainloss_run(items_of_file(gfa_fn), o), gfa_fn, "pan_gainloss");
}

void pg_write_gainloss(pg_graph_t *q, const pg_gainloss_opt_t *o)
{
	if (o == nullptr) { set_error(PGA_ERR_ARG, "pg_write_gainloss"); return; }
	graph_result(gainloss_run(items_of_graph(q), o), "pg_write_gainloss");
}

int pg_pan_gainloss(const uint8_t *presence, int32_t n_item, int32_t n_asm, const int64_t *rec, int32_t method, const pg_gainloss_opt_t *o, int32_t *gene_out,
                    int64_t *node_out)
{
	if (n_item < 0 || n_asm < 0 || (method != PG_TREE_NJ && method != PG_TREE_UPGMA) || (n_asm >= 3 && rec == nullptr) || !gainloss_cost_ok(o)) return PGA_ERR_ARG;
	if (((size_t)n_item * (size_t)n_asm > 0 && presence == nullptr) || (n_item > 0 && gene_out == nullptr) || (n_asm > 0 && node_out == nullptr)) return PGA_ERR_ARG;
	if (n_asm > GAINLOSS_MAX_LEAF || n_item > GAINLOSS_MAX_ITEM) return PGA_ERR_RANGE;
	std::vector<int32_t> kid;
	if (!pairs_tree(rec, n_asm, method, kid)) return PGA_ERR_ARG;
	if (n_asm == 0) { std::fill(gene_out, gene_out + 5 * (size_t)n_item, 0); return 0; } // no tree: nothing is reconstructed
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	t_gainloss = 0;
	return gainloss_core(bits, n_item, n_asm, kid, o->gain, o->loss, o->mode, gene_out, node_out);
}

} // extern "C"
