// pan_coevo.hpp -- co-evolution of the items on the tree of the assemblies (pg_coevo_file, pg_write_coevo, pg_pan_coevo, pangene coevo;
// DESIGN.md section 8 "Co-evolution"): the item pairs whose gains and losses fall on the same branches.  Items, tree and reconstruction
// are pangene gainloss's (pan_gainloss.hpp, included before this header).  The events, the pair counts and the selection run on the
// backend (pga_pan_coevo: reconstruction, event rows, an all-pairs popcount that selects on the device), or as the plain loops below over
// the tree records when the backend has no such entry; the presence counts, r, p_hyper and the table are code both builds share.

namespace pgx {
namespace {

constexpr int32_t COEVO_MAX_ELIG = 4194304; // the backend's limit (include/pangene_hip.h pga_pan_coevo)

// 10^6 d^2 >= p^2 e_i e_j and the sign of d: the definition.  |d| <= B < 2^17, e < 2^17, p <= 1000: both sides < 2^54
inline bool coevo_selected(int64_t d, int64_t ei, int64_t ej, int32_t p, int32_t sign)
{
	if (sign == PG_ASSOC_POS && d < 0) return false;
	if (sign == PG_ASSOC_NEG && d >= 0) return false;
	return (uint64_t)(d * d) * 1000000u >= (uint64_t)(ei * ej) * (uint64_t)((int64_t)p * p);
}

// The backend's step on the host, by the definition and over the tree itself: the states of gainloss_host, per item and branch the
// event x = state[child] - state[parent] (1 a gain, -1 a loss; the branch is named by its lower node, the root has none), then every
// pair of eligible items branch by branch.  bits[A][W], kid as pairs_tree makes it, A >= 2.  events[M] = e_i; pair gets (i, j, same,
// opp) in ascending (i, j) as they are found.  Returns the number selected; only the first max_pair are kept.
int64_t coevo_host(const uint32_t *bits, int32_t M, int32_t A, const std::vector<int32_t> &kid, int32_t g, int32_t l, int32_t mode, int32_t min_events, int32_t p,
                   int32_t sign, int64_t max_pair, std::vector<int32_t> &events, std::vector<int32_t> &pair)
{
	const size_t n_node = (size_t)A + kid.size() / 2, B = n_node - 1;
	std::vector<int32_t> gene(4 * (size_t)M);
	std::vector<int64_t> node(3 * n_node);
	std::vector<uint8_t> states((size_t)M * n_node);
	gainloss_host(bits, M, A, kid, g, l, mode, gene.data(), node.data(), states.data());
	std::vector<int32_t> up(n_node, -1);
	for (size_t t = 0; t < kid.size() / 2; ++t) up[(size_t)kid[2 * t]] = up[(size_t)kid[2 * t + 1]] = A + (int32_t)t;
	events.assign((size_t)M, 0);
	std::vector<int32_t> el; // eligible items
	std::vector<int8_t> X;   // their events, [el.size()][B]
	for (int32_t i = 0; i < M; ++i) {
		const uint8_t *s = states.data() + (size_t)i * n_node;
		int32_t e = 0;
		for (size_t v = 0; v < B; ++v) e += s[v] != s[(size_t)up[v]];
		events[(size_t)i] = e;
		if (e < min_events) continue;
		el.push_back(i);
		for (size_t v = 0; v < B; ++v) X.push_back((int8_t)((int32_t)s[v] - (int32_t)s[(size_t)up[v]]));
	}
	int64_t n = 0;
	pair.clear();
	for (size_t a = 0; a < el.size(); ++a) {
		const int8_t *xa = X.data() + a * B;
		const int64_t ea = events[(size_t)el[a]];
		for (size_t b = a + 1; b < el.size(); ++b) {
			const int8_t *xb = X.data() + b * B;
			int32_t same = 0, opp = 0;
			for (size_t v = 0; v < B; ++v) {
				const int32_t prod = (int32_t)xa[v] * (int32_t)xb[v];
				same += prod > 0, opp += prod < 0;
			}
			if (!coevo_selected((int64_t)same - opp, ea, events[(size_t)el[b]], p, sign)) continue;
			if (n++ < max_pair) pair.push_back(el[a]), pair.push_back(el[b]), pair.push_back(same), pair.push_back(opp);
		}
	}
	return n;
}

double t_coevo = 0; // seconds of the backend step (or the host loops) of the last command

struct CoevoResult { int64_t n = 0; std::vector<int32_t> events, own; const int32_t *pair = nullptr; }; // pair[n][4]

bool coevo_cost_ok(const pg_coevo_opt_t *o)
{
	return o != nullptr && o->gain >= 1 && o->gain <= 255 && o->loss >= 1 && o->loss <= 255 && (o->mode == PG_GAINLOSS_LATE || o->mode == PG_GAINLOSS_EARLY) &&
	       o->min_r >= 0.0 && o->min_r <= 1.0 && o->min_events >= 1 && o->sign >= PG_ASSOC_BOTH && o->sign <= PG_ASSOC_NEG && o->max_pair >= 0;
}

bool coevo_opt_ok(const pg_coevo_opt_t *o)
{
	return coevo_cost_ok(o) && (o->type == PG_DIST_GENE || o->type == PG_DIST_ADJ) && (o->metric == PG_DIST_JACCARD || o->metric == PG_DIST_DIFF) &&
	       (o->method == PG_TREE_NJ || o->method == PG_TREE_UPGMA);
}

// bits[A][W] over M items, the tree of kid (pairs_tree), A >= 2: the events of every item and the selected pairs.  0 or a PGA_ERR_* code;
// r.n is the number of selected pairs in both cases where it is known
int coevo_select(const std::vector<uint32_t> &bits, int32_t M, int32_t A, const std::vector<int32_t> &kid, const pg_coevo_opt_t *o, CoevoResult &r)
{
	r.n = 0, r.pair = nullptr;
	if (A > GAINLOSS_MAX_LEAF || M > GAINLOSS_MAX_ITEM) return PGA_ERR_RANGE;
	const int32_t p = (int32_t)std::floor(1000.0 * o->min_r + 0.5);
	const size_t W = ((size_t)M + 31) / 32;
	const double t0 = now_sec();
	const pga_backend_t *be = backend_default();
	int rc = 0;
	if (be->pan_coevo != nullptr) {
		std::vector<uint8_t> op;
		std::vector<int32_t> node_of, par;
		std::vector<uint32_t> rows;
		if (gainloss_program(bits, W, A, kid, op, node_of, par, rows) > GAINLOSS_DEPTH) return PGA_ERR_RANGE; // (out of reach below 65 536 leaves)
		const pga_coevo_in_t in{op.data(), rows.data(), par.data(), M, A, o->gain, o->loss, o->mode, o->min_events, p, o->sign, o->max_pair, nullptr, 0};
		pga_coevo_out_t res{};
		rc = be->pan_coevo(&in, &res);
		r.n = res.n_pair;
		if (rc == 0) {
			r.pair = res.pair;
			r.events.assign(res.events, res.events + (size_t)M);
		}
	} else {
		r.n = coevo_host(bits.data(), M, A, kid, o->gain, o->loss, o->mode, o->min_events, p, o->sign, o->max_pair, r.events, r.own);
		r.pair = r.own.data();
		if (r.n > o->max_pair) rc = PGA_ERR_RANGE;
		else {
			int64_t n_elig = 0;
			for (const int32_t e : r.events) n_elig += e >= o->min_events;
			if (n_elig > COEVO_MAX_ELIG) rc = PGA_ERR_RANGE;
		}
	}
	t_coevo += now_sec() - t0;
	if (rc == PGA_ERR_RANGE && r.n > o->max_pair)
		std::fprintf(stderr, "Error: %lld item pairs passed, more than the %lld allowed (-x); raise -r or -c\n", (long long)r.n, (long long)o->max_pair);
	return rc;
}

// P(X >= k) for X ~ Hypergeometric(N, a, b) -- b of N branches drawn, a of them marked: lf[i] = log i!, the terms summed from k upwards
// as fisher (trait.cpp) sums its tails
double coevo_hyper(const std::vector<double> &lf, int32_t N, int32_t a, int32_t b, int32_t k)
{
	const int32_t lo = std::max(0, a + b - N), hi = std::min(a, b);
	if (k <= lo) return 1.0;
	const double base = lf[(size_t)a] + lf[(size_t)(N - a)] + lf[(size_t)b] + lf[(size_t)(N - b)] - lf[(size_t)N];
	auto lp = [&](int32_t x) { return base - lf[(size_t)x] - lf[(size_t)(a - x)] - lf[(size_t)(b - x)] - lf[(size_t)(N - a - b + x)]; };
	double sum = 0;
	for (int32_t x = hi; x >= k; --x) sum += std::exp(lp(x));
	return sum < 1.0 ? sum : 1.0;
}

const char *const COEVO_HEADER = "ItemA\tItemB\tnA\tnB\teA\teB\tsame\topp\tr\tp_hyper\n";

// the items, the tree of all assemblies, the events and the pairs, the table
int coevo_run(const ItemSource &src, const pg_coevo_opt_t *o)
{
	const double t_start = now_sec();
	if (!coevo_opt_ok(o)) return PGA_ERR_ARG;
	std::vector<std::string> names, item;
	std::vector<uint32_t> bits;
	int32_t M = 0;
	if (src(o->type, names, bits, M, &item) != 0) return PAN_NO_ITEMS;
	const int32_t A = (int32_t)names.size();
	const double t_prep = now_sec() - t_start;
	OutBuf ob;
	std::string &s = ob.s;
	s = COEVO_HEADER;
	if (A <= 1 || M == 0) { ob.finish(); return 0; }
	if (A > GAINLOSS_MAX_LEAF || M > GAINLOSS_MAX_ITEM) return PGA_ERR_RANGE;
	const double t1 = now_sec();
	std::vector<int64_t> rec((size_t)6 * (size_t)A);
	int rc = tree_joins(bits, M, A, o->metric, o->method, rec.data());
	if (rc != 0) return rc;
	const double t_tree = now_sec() - t1;
	std::vector<int32_t> kid;
	if (!pairs_tree(rec.data(), A, o->method, kid)) return PGA_ERR_ARG;
	CoevoResult r;
	t_coevo = 0;
	if ((rc = coevo_select(bits, M, A, kid, o, r)) != 0) return rc;
	const double t2 = now_sec();
	std::vector<int32_t> present;
	item_counts(bits.data(), M, A, present);
	const int32_t B = 2 * A - 2;
	std::vector<double> lf((size_t)B + 1);
	for (int32_t i = 0; i <= B; ++i) lf[(size_t)i] = std::lgamma((double)i + 1.0);
	char b[160];
	for (int64_t q = 0; q < r.n; ++q) {
		const int32_t *t = r.pair + 4 * q;
		const int32_t i = t[0], j = t[1], same = t[2], opp = t[3], ei = r.events[(size_t)i], ej = r.events[(size_t)j];
		const double rr = (double)(same - opp) / std::sqrt((double)ei * (double)ej);
		s += item[(size_t)i], s += '\t', s += item[(size_t)j];
		std::snprintf(b, sizeof(b), "\t%d\t%d\t%d\t%d\t%d\t%d\t%.4f\t%.3e\n", present[(size_t)i], present[(size_t)j], ei, ej, same, opp, rr, coevo_hyper(lf, B, ei, ej, same + opp));
		s += b;
		ob.flush_if_full();
	}
	ob.finish();
	if (std::getenv("PANGENE_COEVO_TIMING") != nullptr)
		std::fprintf(stderr, "[coevo-timing] route=%s items=%d assemblies=%d pairs=%lld prep_ms=%.3f tree_ms=%.3f select_ms=%.3f write_ms=%.3f all_ms=%.3f\n", src.route(), M, A,
		             (long long)r.n, t_prep * 1e3, t_tree * 1e3, t_coevo * 1e3, (now_sec() - t2) * 1e3, (now_sec() - t_start) * 1e3);
	return 0;
}

} // namespace
} // namespace pgx

extern "C" {

void pg_coevo_opt_init(pg_coevo_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->type = PG_DIST_GENE, o->metric = PG_DIST_JACCARD, o->method = PG_TREE_UPGMA, o->gain = 1, o->loss = 1, o->mode = PG_GAINLOSS_LATE;
	o->min_events = 2, o->sign = PG_ASSOC_BOTH, o->min_r = 0.8, o->max_pair = 16777216;
}

int pg_coevo_file(const char *gfa_fn, const pg_coevo_opt_t *o)
{
	if (o == nullptr) { std::fprintf(stderr, "Error: pan_coevo: no options\n"); return -2; }
	return file_result(coevo_run(items_of_file(gfa_fn), o), gfa_fn, "pan_coevo");
}

void pg_write_coevo(pg_graph_t *q, const pg_coevo_opt_t *o)
{
	if (o == nullptr) { set_error(PGA_ERR_ARG, "pg_write_coevo"); return; }
	graph_result(coevo_run(items_of_graph(q), o), "pg_write_coevo");
}

int64_t pg_pan_coevo(const uint8_t *presence, int32_t n_item, int32_t n_asm, const int64_t *rec, int32_t method, const pg_coevo_opt_t *o, int32_t *events_out,
                     int32_t *pair_out, int64_t cap)
{
	if (n_item < 0 || n_asm < 0 || cap < 0 || (method != PG_TREE_NJ && method != PG_TREE_UPGMA) || (n_asm >= 3 && rec == nullptr) || !coevo_cost_ok(o)) return PGA_ERR_ARG;
	if (((size_t)n_item * (size_t)n_asm > 0 && presence == nullptr) || (cap > 0 && pair_out == nullptr)) return PGA_ERR_ARG;
	if (n_asm > GAINLOSS_MAX_LEAF || n_item > GAINLOSS_MAX_ITEM) return PGA_ERR_RANGE;
	std::vector<int32_t> kid;
	if (!pairs_tree(rec, n_asm, method, kid)) return PGA_ERR_ARG;
	if (events_out != nullptr) std::fill(events_out, events_out + (size_t)n_item, 0);
	if (n_asm <= 1 || n_item == 0) return 0; // no branch: no events
	std::vector<uint32_t> bits;
	pack_cols(presence, n_item, n_asm, bits);
	CoevoResult r;
	t_coevo = 0;
	const int rc = coevo_select(bits, n_item, n_asm, kid, o, r);
	if (rc != 0) return rc;
	if (events_out != nullptr) std::copy(r.events.begin(), r.events.end(), events_out);
	const int64_t n = r.n < cap ? r.n : cap;
	if (n > 0) std::memcpy(pair_out, r.pair, sizeof(int32_t) * 4 * (size_t)n);
	return r.n;
}

} // extern "C"
