// pan_treeprog.hpp -- the records of a tree as a binary tree, and that tree as the postfix program the backend's tree dynamic programmes
// run (pga_pan_pairs, pga_pan_gainloss): what pangene trait -L (trait.cpp) and pangene gainloss (pan_gainloss.hpp in tree.cpp) share, so
// that both commands read records, and NJ's closing trifurcation, through one compiler.  Included after pg_internal.hpp.
#pragma once

namespace pgx {
namespace {

// The records of pg_pan_tree / pg_pan_join as a binary tree: node x < A is leaf x, node A + t the t-th join with the children
// kid[2 t] (the subtree of slot i) and kid[2 t + 1] (of slot j); joins are numbered in record order, so a child's number is below its
// parent's and the root is the last node.  NJ's closing record (x, y, z) is read as ((x, y), z).  One leaf is a tree, two are one
// join; neither needs records.  false: the records name a slot out of range, twice in a join, or one that has retired.
bool pairs_tree(const int64_t *rec, int32_t A, int32_t method, std::vector<int32_t> &kid)
{
	kid.clear();
	if (A < 2) return true;
	if (A == 2) { kid = {0, 1}; return true; }
	if (rec == nullptr) return false;
	std::vector<int32_t> at((size_t)A);
	for (int32_t x = 0; x < A; ++x) at[(size_t)x] = x;
	auto join = [&](int64_t i, int64_t j) {
		if (i < 0 || j < 0 || i >= A || j >= A || i == j || at[(size_t)i] < 0 || at[(size_t)j] < 0) return false;
		kid.push_back(at[(size_t)i]), kid.push_back(at[(size_t)j]);
		at[(size_t)i] = A + (int32_t)(kid.size() / 2) - 1, at[(size_t)j] = -1;
		return true;
	};
	const int32_t n_plain = method == PG_TREE_NJ ? A - 3 : A - 1;
	for (int32_t t = 0; t < n_plain; ++t)
		if (!join(rec[6 * (size_t)t], rec[6 * (size_t)t + 1])) return false;
	if (method == PG_TREE_NJ) {
		const int64_t *fin = rec + 6 * (size_t)n_plain;
		if (!join(fin[0], fin[1]) || !join(fin[0], fin[2])) return false;
	}
	return true;
}

// The tree as the backend's postfix program: op 0 pushes the next leaf (order[k] = the k-th pushed leaf), op 1 joins the top two
// entries.  A join visits the child that needs the deeper stack first (the Ershov number: a leaf needs 1, a join of two equal needs one
// more, of two unequal the larger), ties the subtree of slot i: the stack then never holds more than floor(log2 A) + 1 entries.  Returns
// that need of the root.
int32_t pairs_program(const std::vector<int32_t> &kid, int32_t A, std::vector<uint8_t> &op, std::vector<int32_t> &order)
{
	op.clear(), order.clear();
	if (A == 0) return 0;
	const size_t n_join = kid.size() / 2;
	std::vector<int32_t> need((size_t)A + n_join, 1);
	for (size_t t = 0; t < n_join; ++t) {
		const int32_t a = need[(size_t)kid[2 * t]], b = need[(size_t)kid[2 * t + 1]];
		need[(size_t)A + t] = a == b ? a + 1 : std::max(a, b);
	}
	std::vector<int32_t> todo; // a node to visit, or ~node: emit its join
	todo.push_back((int32_t)((size_t)A + n_join) - 1);
	while (!todo.empty()) {
		const int32_t v = todo.back();
		todo.pop_back();
		if (v < 0) op.push_back(1);
		else if (v < A) op.push_back(0), order.push_back(v);
		else {
			const int32_t a = kid[2 * (size_t)(v - A)], b = kid[2 * (size_t)(v - A) + 1];
			const bool a_first = need[(size_t)a] >= need[(size_t)b];
			todo.push_back(~v), todo.push_back(a_first ? b : a), todo.push_back(a_first ? a : b);
		}
	}
	return need.back();
}

} // namespace
} // namespace pgx
