// call.cpp -- pangene.js `call` (version 1.1-r231; pangene.js:93-392 for the GFA side, 440-980 for the net graph, the program
// structure tree and the walk side), bubble calling on the gene graph, byte for byte.
//
// Graph side (host, sequential -- it scales with segments, not genomes): the script's GFA reader, the net graph whose nodes are
// the segment ends that links join, Johnson's cycle equivalence on it (mark_cec), bubble discovery by a BFS from every vertex
// (get_bubble_all) or, with -p, the program structure tree.  The script shares its flag arrays between the starts of the
// discovery (a flag value of one start can equal the value of a later one), so the starts run in order, as there.
// Walk side (pga_call_bubbles on the backend; the plain loops below when the backend has none): which walks pass through which
// bubble, the alleles they take, the genes inside.
#include <climits>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>
#include "pg_internal.hpp"

namespace pgx {
namespace {

struct CallError : std::runtime_error { using std::runtime_error::runtime_error; };

// JavaScript parseInt on a decimal string: leading blanks, a sign, digits; no digit = NaN.  Returns false for NaN.
bool js_parse_int(const char *s, int64_t &v)
{
	while (*s == ' ' || *s == '\t' || *s == '\n' || *s == '\r' || *s == '\f' || *s == '\v') ++s;
	bool neg = false;
	if (*s == '+' || *s == '-') neg = *s++ == '-';
	if (*s < '0' || *s > '9') return false;
	int64_t x = 0;
	for (; *s >= '0' && *s <= '9'; ++s) if (x < ((int64_t)1 << 40)) x = x * 10 + (*s - '0');
	v = neg ? -x : x;
	return true;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the graph as the script reads it
// ---------------------------------------------------------------------------------------------------------------------------
struct Graph {
	std::vector<std::string> name;              // segment names, ids by first appearance (S-lines, then L-lines)
	std::unordered_map<std::string, int32_t> id;
	struct Arc { int32_t v, w; bool rank0; };
	std::vector<Arc> arc;                       // L-lines in file order, then stably by source vertex, SR:i:0 first per vertex
	std::vector<int64_t> off;                   // arcs of vertex v: [off[v], off[v+1])
	std::vector<std::string> walk_asm;          // "sample#hap" per W-line
	std::vector<int32_t> step;                  // the walks' known steps, concatenated
	std::vector<int64_t> walk_off{0};
	std::vector<int32_t> cec;                   // per segment, set by the cycle equivalence (-1: none)

	int32_t n_seg() const { return (int32_t)name.size(); }
	int32_t n_vtx() const { return 2 * n_seg(); }
	int32_t seg_add(const std::string &s) {
		auto it = id.find(s);
		if (it != id.end()) return it->second;
		id.emplace(s, n_seg());
		name.push_back(s);
		return n_seg() - 1;
	}
	// sort the arcs stably by source vertex, build the vertex index, move the last SR:i:0 arc of every vertex to its front
	void index() {
		std::stable_sort(arc.begin(), arc.end(), [](const Arc &a, const Arc &b) { return a.v < b.v; });
		off.assign((size_t)n_vtx() + 1, 0);
		for (const Arc &a : arc) ++off[(size_t)a.v + 1];
		for (int32_t v = 0; v < n_vtx(); ++v) off[(size_t)v + 1] += off[(size_t)v];
		for (int32_t v = 0; v < n_vtx(); ++v) {
			int64_t last0 = -1;
			for (int64_t i = off[(size_t)v]; i < off[(size_t)v + 1]; ++i) if (arc[(size_t)i].rank0) last0 = i;
			if (last0 > off[(size_t)v]) std::swap(arc[(size_t)off[(size_t)v]], arc[(size_t)last0]);
		}
		cec.assign((size_t)n_seg(), -1);
	}
	int64_t n_out(int32_t v) const { return off[(size_t)v + 1] - off[(size_t)v]; }
};

void split_tab(const std::string &l, std::vector<std::string> &t)
{
	t.clear();
	for (size_t b = 0;;) {
		const size_t e = l.find('\t', b);
		t.push_back(l.substr(b, e == std::string::npos ? std::string::npos : e - b));
		if (e == std::string::npos) break;
		b = e + 1;
	}
}

void parse_gfa(const std::vector<std::string> &lines, Graph &g)
{
	std::vector<std::string> t;
	for (const std::string &l : lines) {
		if (l.empty()) continue;
		if (l[0] == 'S') {
			split_tab(l, t);
			if (t.size() >= 3) g.seg_add(t[1]);
		} else if (l[0] == 'L') {
			split_tab(l, t);
			if (t.size() < 5 || (t[2] != "+" && t[2] != "-") || (t[4] != "+" && t[4] != "-")) continue;
			const int32_t s1 = g.seg_add(t[1]), s2 = g.seg_add(t[3]);
			bool rank0 = false;
			for (size_t j = 6; j < t.size(); ++j) { // the last SR:i tag counts
				if (t[j].compare(0, 5, "SR:i:") != 0 || t[j].size() == 5 || std::isspace((unsigned char)t[j][5])) continue;
				int64_t r;
				rank0 = js_parse_int(t[j].c_str() + 5, r) && r == 0;
			}
			g.arc.push_back({s1 * 2 + (t[2] == "-"), s2 * 2 + (t[4] == "-"), rank0});
		} else if (l[0] == 'W') {
			split_tab(l, t);
			if (t.size() < 7) continue;
			g.walk_asm.push_back(t[1] + "#" + t[2]);
			const std::string &w = t[6];
			for (size_t i = 0; i < w.size();) { // ([><])([^\s><]+): unknown names are dropped
				if (w[i] != '>' && w[i] != '<') { ++i; continue; }
				size_t e = i + 1;
				while (e < w.size() && w[e] != '>' && w[e] != '<' && !std::isspace((unsigned char)w[e])) ++e;
				if (e > i + 1) {
					auto it = g.id.find(w.substr(i + 1, e - i - 1));
					if (it != g.id.end()) g.step.push_back(it->second * 2 + (w[i] == '<'));
				}
				i = e;
			}
			g.walk_off.push_back((int64_t)g.step.size());
		}
	}
	g.index();
}

// ---------------------------------------------------------------------------------------------------------------------------
// bubbles
// ---------------------------------------------------------------------------------------------------------------------------
struct Bubble {
	int32_t cec = -1, par = -1, vs = -1, ve = -1;
	bool flt = false;
	std::vector<int32_t> seg;                   // interior segments as discovered (the BB line of the third form lists them)
	// walk side
	bool has_walks = false;
	int32_t n_gene = 0;
	std::vector<int32_t> gene;                  // interior segments in order of first appearance (empty over max_ext)
	struct Allele { int32_t n; int64_t rec; std::vector<int32_t> walks; };
	std::vector<Allele> al;
};

// Reachability of ve from vs without crossing back over vs or onto ve's other strand; the interior segments found, [] when
// there is no bubble or more than max_n of them.  flag[] is shared with the caller: a vertex is "seen" when it holds f.
std::vector<int32_t> reach(const Graph &g, int32_t vs, int32_t ve, std::vector<int64_t> &flag, int64_t f, int64_t max_n)
{
	std::vector<int32_t> stack{vs}, list;
	flag[(size_t)vs] = f;
	while (!stack.empty()) {
		const int32_t v = stack.back();
		stack.pop_back();
		for (int64_t i = g.off[(size_t)v]; i < g.off[(size_t)v + 1]; ++i) {
			const int32_t w = g.arc[(size_t)i].w;
			if (w == (vs ^ 1)) continue;
			if (w == (ve ^ 1)) return {};
			if (flag[(size_t)w] == f) continue;
			flag[(size_t)w] = f;
			if (w == ve) continue;
			if (flag[(size_t)(w ^ 1)] != f) list.push_back(w >> 1);
			stack.push_back(w);
		}
		if ((int64_t)list.size() > max_n) break;
	}
	if ((int64_t)list.size() > max_n) return {};
	return list;
}

std::vector<int32_t> bubble_between(const Graph &g, int32_t vs, int32_t ve, std::vector<int64_t> &flag, int64_t f, int64_t max_n)
{
	const int64_t ff = f, fr = f + g.n_vtx();
	std::vector<int32_t> fw = reach(g, vs, ve, flag, ff, max_n);
	std::vector<int32_t> rv = reach(g, ve ^ 1, vs ^ 1, flag, fr, max_n);
	if (fw.size() != rv.size()) return {};
	for (int32_t s : fw)
		if (flag[(size_t)s * 2] != fr && flag[(size_t)s * 2 + 1] != fr) return {};
	for (int32_t s : fw)
		for (int32_t v = s * 2; v <= s * 2 + 1; ++v)
			for (int64_t i = g.off[(size_t)v]; i < g.off[(size_t)v + 1]; ++i) {
				const int64_t x = flag[(size_t)g.arc[(size_t)i].w];
				if (x != ff && x != fr) return {};
			}
	return fw;
}

// Array.prototype.sort() without a comparator compares the decimal strings: 10 < 100 < 9
bool decimal_less(int32_t a, int32_t b)
{
	char sa[16], sb[16];
	std::snprintf(sa, sizeof(sa), "%d", a), std::snprintf(sb, sizeof(sb), "%d", b);
	return std::strcmp(sa, sb) < 0;
}

// vertices one link away in either direction (successors of v, and the other successors of those successors' predecessors),
// in decimal-string order without repeats
void undirected_neighbors(const Graph &g, int32_t v, std::vector<int32_t> &a)
{
	a.clear();
	for (int64_t i = g.off[(size_t)v]; i < g.off[(size_t)v + 1]; ++i) {
		const int32_t w = g.arc[(size_t)i].w;
		a.push_back(w);
		for (int64_t j = g.off[(size_t)(w ^ 1)]; j < g.off[(size_t)(w ^ 1) + 1]; ++j)
			if (g.arc[(size_t)j].w != (v ^ 1)) a.push_back(g.arc[(size_t)j].w);
	}
	std::stable_sort(a.begin(), a.end(), decimal_less);
	a.erase(std::unique(a.begin(), a.end()), a.end());
}

std::vector<Bubble> bubbles_by_bfs(const Graph &g, int64_t max_ext)
{
	const int32_t nv = g.n_vtx();
	std::vector<int64_t> flag1((size_t)nv, -1), flag2((size_t)nv, -1);
	int64_t f1 = 0, f2 = 0;
	std::vector<Bubble> bb;
	std::vector<int32_t> queue, ends, nei;
	for (int32_t vs = 0; vs < nv; ++vs) {
		const int32_t cec = g.cec[(size_t)(vs >> 1)];
		if (cec < 0 || g.n_out(vs) == 0) continue;
		if (g.n_out(vs) == 1 && g.n_out(g.arc[(size_t)g.off[(size_t)vs]].w ^ 1) < 2) continue;
		queue.assign(1, vs), ends.clear();
		size_t head = 0;
		int64_t ext = 0;
		flag1[(size_t)vs] = f1;
		while (head < queue.size()) {
			undirected_neighbors(g, queue[head++], nei);
			for (int32_t w : nei) {
				if (flag1[(size_t)w] == f1) continue;
				if (flag1[(size_t)(w ^ 1)] != f1) ++ext;
				if (w == (vs ^ 1)) continue;
				flag1[(size_t)w] = f1;
				if (g.cec[(size_t)(w >> 1)] == cec) ends.push_back(w);
				else queue.push_back(w);
			}
			if (ext > max_ext) break;
		}
		for (int32_t ve : ends) {
			std::vector<int32_t> r = bubble_between(g, vs, ve, flag2, f2, max_ext);
			if (!r.empty() && vs < ve) {
				Bubble b;
				b.cec = cec, b.vs = vs, b.ve = ve, b.seg = std::move(r);
				bb.push_back(std::move(b));
			}
			++f2;
		}
		++f1;
	}
	// parents: the largest bubbles first (stable), every segment remembers the last bubble that covered it
	std::vector<int32_t> order(bb.size());
	for (size_t i = 0; i < bb.size(); ++i) order[i] = (int32_t)i;
	std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return bb[(size_t)a].seg.size() > bb[(size_t)b].seg.size(); });
	std::vector<int32_t> owner((size_t)g.n_seg(), -1);
	for (int32_t id : order) {
		Bubble &b = bb[(size_t)id];
		int32_t par = -2;
		bool nested = true;
		for (int32_t s : b.seg) {
			if (par == -2) par = owner[(size_t)s];
			else if (par != owner[(size_t)s]) nested = false;
			owner[(size_t)s] = id;
		}
		b.par = nested ? par : -2;
	}
	return bb;
}

// ---------------------------------------------------------------------------------------------------------------------------
// the net graph: a node per class of segment ends that links join, an edge per segment in each direction
// ---------------------------------------------------------------------------------------------------------------------------
struct Net {
	const Graph &g;
	struct Edge { int32_t v, w, seg, ori, pair, cec, type; }; // type 0 unseen, 1 tree, 2 back, 3 blocked
	int32_t n_node = 0;
	std::vector<Edge> e;
	std::vector<int64_t> off;
	std::vector<int32_t> dis, fin, par;

	Net(const Graph &gg, bool add_super, const char *ref) : g(gg) { build(add_super, ref); }

	void build(bool add_super, const char *ref) {
		const int32_t nv = g.n_vtx(), ns = g.n_seg();
		// end-to-end links: (v^1, w) for every arc v -> w, stably by the first end
		std::vector<std::pair<int32_t, int32_t>> lk;
		for (int32_t v = 0; v < nv; ++v)
			for (int64_t i = g.off[(size_t)v]; i < g.off[(size_t)v + 1]; ++i) lk.emplace_back(v ^ 1, g.arc[(size_t)i].w);
		std::stable_sort(lk.begin(), lk.end(), [](const std::pair<int32_t, int32_t> &a, const std::pair<int32_t, int32_t> &b) { return a.first < b.first; });
		std::vector<int64_t> lo((size_t)nv + 1, 0);
		for (auto &x : lk) ++lo[(size_t)x.first + 1];
		for (int32_t v = 0; v < nv; ++v) lo[(size_t)v + 1] += lo[(size_t)v];
		// classes, following the links forward only: a class reached from two starts means the links were listed one way
		std::vector<int32_t> cat((size_t)nv, -1), stack;
		int32_t x = 0;
		for (int32_t v = 0; v < nv; ++v) {
			if (cat[(size_t)v] >= 0) continue;
			stack.assign(1, v);
			while (!stack.empty()) {
				const int32_t w = stack.back();
				stack.pop_back();
				cat[(size_t)w] = x;
				for (int64_t i = lo[(size_t)w]; i < lo[(size_t)w + 1]; ++i) {
					const int32_t u = lk[(size_t)i].second;
					if (cat[(size_t)u] < 0) cat[(size_t)u] = x, stack.push_back(u);
					else if (cat[(size_t)u] != x) throw CallError("Wrong!");
				}
			}
			++x;
		}
		n_node = x;
		for (int32_t s = 0; s < ns; ++s) {
			e.push_back({cat[(size_t)s * 2], cat[(size_t)s * 2 + 1], s, 1, -1, -1, 0});
			e.push_back({cat[(size_t)s * 2 + 1], cat[(size_t)s * 2], s, -1, -1, -1, 0});
		}
		if (add_super) {
			std::vector<int32_t> tip;
			for (int32_t v = 0; v < nv; ++v) if (g.n_out(v) == 0) tip.push_back(v ^ 1);
			if (ref != nullptr && !g.walk_asm.empty()) {
				std::vector<uint8_t> f((size_t)nv, 0);
				for (int32_t t : tip) f[(size_t)t] = 1;
				for (size_t j = 0; j < g.walk_asm.size(); ++j) {
					const int64_t a = g.walk_off[j], b = g.walk_off[j + 1];
					if (g.walk_asm[j] != ref || b - a < 2) continue;
					const int32_t t1 = g.step[(size_t)a], t2 = g.step[(size_t)b - 1] ^ 1;
					if (f[(size_t)t1] == 0) f[(size_t)t1] = 2;
					if (f[(size_t)t2] == 0) f[(size_t)t2] = 2;
				}
				for (int32_t v = 0; v < nv; ++v) if (f[(size_t)v] == 2) tip.push_back(v);
			}
			if (!tip.empty()) {
				const int32_t sn = n_node++;
				int32_t sid = ns;
				for (int32_t v : tip) {
					e.push_back({sn, cat[(size_t)v], sid, 1, -1, -1, 0});
					e.push_back({cat[(size_t)v], sn, sid, -1, -1, -1, 0});
					++sid;
				}
			}
		}
		std::stable_sort(e.begin(), e.end(), [](const Edge &a, const Edge &b) { return a.v < b.v; });
		off.assign((size_t)n_node + 1, 0);
		for (const Edge &a : e) ++off[(size_t)a.v + 1];
		for (int32_t v = 0; v < n_node; ++v) off[(size_t)v + 1] += off[(size_t)v];
		// the two directions of a segment (or of a link to the super node, numbered after the segments) pair up
		std::vector<int32_t> of(e.size() + 2, -1);
		for (size_t i = 0; i < e.size(); ++i) of[(size_t)e[i].seg * 2 + (e[i].ori < 0)] = (int32_t)i;
		for (size_t i = 0; i < e.size(); ++i) e[i].pair = of[(size_t)e[i].seg * 2 + (e[i].ori > 0)];
	}
	Edge &pair_of(const Edge &a) {
		if (a.pair < 0) throw CallError("Cannot read properties of undefined");
		return e[(size_t)a.pair];
	}

	void dfs_from(int32_t v, int32_t &t_dis, int32_t &t_fin, std::vector<uint8_t> &state) {
		if (state[(size_t)v] != 0) return;
		dis[(size_t)v] = t_dis++;
		state[(size_t)v] = 2;
		std::vector<std::pair<int32_t, int64_t>> stack{{v, 0}};
		while (!stack.empty()) {
			const auto [w, i] = stack.back();
			stack.pop_back();
			if (i < off[(size_t)w + 1] - off[(size_t)w]) {
				Edge &a = e[(size_t)(off[(size_t)w] + i)];
				stack.push_back({w, i + 1});
				if (a.type == 3) continue;
				const int32_t u = a.w;
				if (state[(size_t)u] == 0) {
					state[(size_t)u] = 2;
					dis[(size_t)u] = t_dis++;
					par[(size_t)u] = w;
					stack.push_back({u, 0});
					a.type = 1;
					pair_of(a).type = 3;
				} else if (state[(size_t)u] == 2) {
					a.type = 2;
					pair_of(a).type = 3;
				}
			} else {
				state[(size_t)w] = 1;
				fin[(size_t)w] = t_fin++;
			}
		}
	}
	void dfs() {
		dis.assign((size_t)n_node, -1), fin.assign((size_t)n_node, -1), par.assign((size_t)n_node, -1);
		std::vector<uint8_t> state((size_t)n_node, 0);
		int32_t td = 0, tf = 0;
		if (n_node > 0) dfs_from(n_node - 1, td, tf, state);
		for (int32_t v = 0; v < n_node; ++v) if (state[(size_t)v] == 0) dfs_from(v, td, tf, state);
		if (td != n_node || tf != n_node) throw CallError("DFS bug");
	}
	std::vector<int32_t> by_discovery() const {
		std::vector<int32_t> o((size_t)n_node);
		for (int32_t v = 0; v < n_node; ++v) o[(size_t)dis[(size_t)v]] = v;
		return o;
	}

	// Cycle equivalence of the edges (Johnson, Pearson, Pingali 1994, with the script's capping rule); returns the number of classes.
	int32_t mark_cec() {
		dfs();
		const std::vector<int32_t> vd = by_discovery();
		// bracket lists: intrusive doubly linked lists of nodes in one pool
		struct Node { int64_t a; int32_t recent_size = -1, recent_cec = -1, prev = -1, next = -1; };
		struct List { int32_t head = -1, tail = -1, size = 0; };
		std::vector<Node> pool;
		auto push = [&](List &l, int32_t n) {
			if (l.head < 0 && l.tail < 0) l.head = l.tail = n;
			else pool[(size_t)l.tail].next = n, pool[(size_t)n].prev = l.tail, l.tail = n;
			++l.size;
		};
		auto append = [&](List &l, const List &m) {
			if (m.head < 0 && m.tail < 0) return;
			if (l.head < 0 && l.tail < 0) l.head = m.head, l.tail = m.tail;
			else pool[(size_t)l.tail].next = m.head, pool[(size_t)m.head].prev = l.tail, l.tail = m.tail;
			l.size += m.size;
		};
		auto remove = [&](List &l, int32_t n) {
			Node &x = pool[(size_t)n];
			if (l.head == n && l.tail == n) l.head = l.tail = -1;
			else if (l.tail == n) l.tail = x.prev, pool[(size_t)l.tail].next = -1;
			else if (l.head == n) l.head = x.next, pool[(size_t)l.head].prev = -1;
			else pool[(size_t)x.prev].next = x.next, pool[(size_t)x.next].prev = x.prev;
			--l.size;
		};
		struct Vs { int32_t hi; List bl; std::vector<int32_t> be_end, be_cap; };
		std::vector<Vs> vs((size_t)n_node);
		for (auto &x : vs) x.hi = n_node;
		int32_t cec = 1;
		for (int32_t t = (int32_t)vd.size() - 1; t >= 0; --t) {
			const int32_t v = vd[(size_t)t];
			const int64_t o = off[(size_t)v], n = off[(size_t)v + 1] - o;
			int32_t hi0 = n_node;
			for (int64_t i = 0; i < n; ++i) {
				const Edge &a = e[(size_t)(o + i)];
				if (a.type != 2 || a.w == v) continue;
				hi0 = std::min(hi0, dis[(size_t)a.w]);
			}
			int32_t hi1 = n_node, hi2 = n_node;
			List bl;
			for (int64_t i = 0; i < n; ++i) {
				const Edge &a = e[(size_t)(o + i)];
				if (a.type != 1) continue;
				const int32_t h = vs[(size_t)a.w].hi;
				if (hi1 > h) hi2 = hi1, hi1 = h;
				else if (hi2 > h) hi2 = h;
				append(bl, vs[(size_t)a.w].bl);
			}
			vs[(size_t)v].hi = std::min(hi0, hi1);
			for (int32_t b : vs[(size_t)v].be_cap) remove(bl, b);
			for (int32_t b : vs[(size_t)v].be_end) {
				remove(bl, b);
				Edge &a = e[(size_t)pool[(size_t)b].a];
				if (a.cec < 0) a.cec = cec++;
			}
			for (int64_t i = 0; i < n; ++i) {
				const Edge &a = e[(size_t)(o + i)];
				if (a.type != 2 || a.w == v) continue;
				pool.push_back(Node{o + i});
				push(bl, (int32_t)pool.size() - 1);
				vs[(size_t)a.w].be_end.push_back((int32_t)pool.size() - 1);
			}
			if (hi2 < hi0 && hi2 < t) {
				pool.push_back(Node{-1});
				push(bl, (int32_t)pool.size() - 1);
				vs[(size_t)vd[(size_t)hi2]].be_cap.push_back((int32_t)pool.size() - 1);
			}
			vs[(size_t)v].bl = bl;
			if (par[(size_t)v] >= 0) {
				const int32_t u = par[(size_t)v];
				int64_t te = -1;
				for (int64_t i = off[(size_t)u]; i < off[(size_t)u + 1]; ++i)
					if (e[(size_t)i].w == v && e[(size_t)i].type == 1) te = i;
				if (te < 0) throw CallError("Bug: failed to find tree edge");
				if (bl.size > 0) {
					Node &b = pool[(size_t)bl.tail];
					if (b.recent_size != bl.size) b.recent_size = bl.size, b.recent_cec = cec++;
					if (b.recent_cec < 0) throw CallError("Bug: recent_cec not set");
					e[(size_t)te].cec = b.recent_cec;
					if (b.recent_size == 1 && b.a >= 0) e[(size_t)b.a].cec = e[(size_t)te].cec;
				} else e[(size_t)te].cec = 0;
			}
		}
		std::vector<int32_t> &sc = const_cast<Graph &>(g).cec;
		for (const Edge &a : e)
			if (a.seg < g.n_seg() && (a.type == 1 || a.type == 2)) sc[(size_t)a.seg] = a.cec;
		return cec;
	}

	// the program structure tree: SESE regions from one DFS, then open regions, regions at the super node and point regions
	// removed (their children move up to the nearest region kept)
	std::vector<Bubble> pst() {
		const int32_t n_cec = mark_cec();
		const std::vector<int32_t> vd = by_discovery();
		struct Sese { int32_t cec; int64_t st, en; int32_t par, unflt, i; };
		std::vector<Sese> se;
		std::vector<int32_t> entry((size_t)n_cec, -1);
		std::vector<uint8_t> seen((size_t)n_node, 0);
		struct Fr { int32_t w; int64_t i; int32_t b; };
		std::vector<Fr> stack;
		for (int32_t v : vd) {
			if (seen[(size_t)v]) continue;
			seen[(size_t)v] = 1;
			stack.assign(1, Fr{v, 0, -1});
			while (!stack.empty()) {
				const Fr f = stack.back();
				stack.pop_back();
				const int64_t o = off[(size_t)f.w], n = off[(size_t)f.w + 1] - o;
				if (f.i == n) continue;
				stack.push_back(Fr{f.w, f.i + 1, f.b});
				const Edge &a = e[(size_t)(o + f.i)];
				if (a.type == 3) continue;
				int32_t b2 = f.b;
				if (a.cec >= 0) {
					int32_t p = f.b;
					int32_t &open = entry[(size_t)a.cec];
					if (open != -1) se[(size_t)open].en = o + f.i, p = se[(size_t)open].par;
					se.push_back(Sese{a.cec, o + f.i, -1, p, -1, -1});
					b2 = open = (int32_t)se.size() - 1;
				}
				if (seen[(size_t)a.w]) continue;
				seen[(size_t)a.w] = 1;
				stack.push_back(Fr{a.w, 0, b2});
			}
		}
		std::vector<Bubble> out;
		for (size_t i = 0; i < se.size(); ++i) {
			Sese &b = se[i];
			bool drop = false;
			if (b.en < 0) drop = true;
			else if (e[(size_t)b.st].seg >= g.n_seg() || e[(size_t)b.en].seg >= g.n_seg()) drop = true;
			else if (e[(size_t)b.st].w == e[(size_t)b.en].v && off[(size_t)e[(size_t)b.en].v + 1] - off[(size_t)e[(size_t)b.en].v] == 2) drop = true;
			if (drop) {
				b.unflt = b.par >= 0 ? se[(size_t)b.par].unflt : -1;
				continue;
			}
			b.unflt = (int32_t)i;
			if (b.par >= 0) b.par = se[(size_t)b.par].unflt;
			b.i = (int32_t)out.size();
			Bubble x;
			x.cec = b.cec, x.par = b.par < 0 ? -1 : se[(size_t)b.par].i;
			const Edge &s = e[(size_t)b.st], &t = e[(size_t)b.en];
			x.vs = s.seg * 2 + (s.ori > 0 ? 0 : 1), x.ve = t.seg * 2 + (t.ori > 0 ? 0 : 1);
			out.push_back(std::move(x));
		}
		return out;
	}
};

// ---------------------------------------------------------------------------------------------------------------------------
// the walk side without a backend entry: the script's own procedure (one pass over every walk, an "open starts" list per end
// vertex that is reset at the first start of a new walk), then the alleles and genes with hash maps
// ---------------------------------------------------------------------------------------------------------------------------
struct WalkSide {
	std::vector<pga_call_rec_t> rec;
	std::vector<int32_t> rep, cnt, gene_bub, gene_seg;
	std::vector<int64_t> gene_first;
};

void walk_side_host(const pga_call_in_t &in, WalkSide &ws)
{
	const int32_t nv = in.n_seg * 2;
	struct St { int32_t en, bo; };
	std::vector<std::vector<St>> starts((size_t)nv);
	for (int32_t b = 0; b < in.n_bub; ++b) {
		if (in.bub_vs[b] < 0) continue;
		starts[(size_t)in.bub_vs[b]].push_back({in.bub_ve[b], b * 2});
		starts[(size_t)(in.bub_ve[b] ^ 1)].push_back({in.bub_vs[b] ^ 1, b * 2 + 1});
	}
	struct Open { int32_t st_off, bo; };
	std::vector<int32_t> open_walk((size_t)nv, -1);
	std::vector<std::vector<Open>> open((size_t)nv);
	std::vector<std::vector<pga_call_rec_t>> per((size_t)in.n_bub);
	for (int32_t j = 0; j < in.n_walk; ++j) {
		const int32_t *w = in.step + in.walk_off[j];
		const int32_t len = (int32_t)(in.walk_off[j + 1] - in.walk_off[j]);
		for (int32_t i = 0; i < len; ++i) {
			const int32_t v = w[i];
			for (const St &s : starts[(size_t)v]) {
				if (open_walk[(size_t)s.en] != j) open_walk[(size_t)s.en] = j, open[(size_t)s.en].clear();
				open[(size_t)s.en].push_back({i, s.bo});
			}
			if (open_walk[(size_t)v] != j) continue;
			for (const Open &o : open[(size_t)v]) per[(size_t)(o.bo >> 1)].push_back({o.bo, j, o.st_off, i});
		}
	}
	for (auto &p : per) ws.rec.insert(ws.rec.end(), p.begin(), p.end());
	const int64_t n = (int64_t)ws.rec.size();
	ws.rep.assign((size_t)n, -1), ws.cnt.assign((size_t)n, 0);
	std::vector<int32_t> path;
	for (int64_t r0 = 0, ig = 0; r0 < n;) {
		const int32_t b = ws.rec[(size_t)r0].bo >> 1;
		int64_t r1 = r0;
		while (r1 < n && ws.rec[(size_t)r1].bo >> 1 == b) ++r1;
		std::unordered_map<std::string, int64_t> first;
		std::unordered_map<int32_t, size_t> gpos;
		const size_t g0 = ws.gene_seg.size();
		for (int64_t r = r0; r < r1; ++r) {
			const pga_call_rec_t &x = ws.rec[(size_t)r];
			const int32_t *w = in.step + in.walk_off[x.walk];
			for (int32_t k = x.st_off + 1; k < x.en_off; ++k, ++ig)
				if (gpos.emplace(w[k] >> 1, ws.gene_seg.size()).second) ws.gene_bub.push_back(b), ws.gene_seg.push_back(w[k] >> 1), ws.gene_first.push_back(ig);
			path.clear();
			if ((x.bo & 1) == 0) for (int32_t k = x.st_off; k <= x.en_off; ++k) path.push_back(w[k]);
			else for (int32_t k = x.en_off; k >= x.st_off; --k) path.push_back(w[k] ^ 1);
			const std::string key((const char *)path.data(), path.size() * sizeof(int32_t));
			const int64_t f = first.emplace(key, r).first->second;
			ws.rep[(size_t)r] = (int32_t)f, ++ws.cnt[(size_t)f];
		}
		// (bubble, segment) order, as the backend returns them
		std::vector<size_t> o(ws.gene_seg.size() - g0);
		for (size_t i = 0; i < o.size(); ++i) o[i] = g0 + i;
		std::sort(o.begin(), o.end(), [&](size_t a, size_t c) { return ws.gene_seg[a] < ws.gene_seg[c]; });
		std::vector<int32_t> s2(o.size());
		std::vector<int64_t> f2(o.size());
		for (size_t i = 0; i < o.size(); ++i) s2[i] = ws.gene_seg[o[i]], f2[i] = ws.gene_first[o[i]];
		std::copy(s2.begin(), s2.end(), ws.gene_seg.begin() + (ptrdiff_t)g0);
		std::copy(f2.begin(), f2.end(), ws.gene_first.begin() + (ptrdiff_t)g0);
		r0 = r1;
	}
}

// fills the walk side of every bubble: records on the backend (or the loops above), then alleles in order of first appearance,
// stably by support, and the genes, in order of first appearance
void walk_side(const Graph &g, std::vector<Bubble> &bb, int64_t max_ext)
{
	std::vector<int32_t> vs(bb.size()), ve(bb.size());
	for (size_t i = 0; i < bb.size(); ++i) {
		vs[i] = bb[i].flt ? -1 : bb[i].vs, ve[i] = bb[i].ve;
		bb[i].has_walks = true;
	}
	pga_call_in_t in{g.step.data(), g.walk_off.data(), (int32_t)g.walk_asm.size(), g.n_seg(), vs.data(), ve.data(), (int32_t)bb.size()};
	pga_call_out_t out{};
	WalkSide host;
	const pga_backend_t *be = backend_default();
	if (be->call_bubbles != nullptr) {
		const int rc = be->call_bubbles(&in, &out);
		if (rc != 0) throw CallError(std::string("call_bubbles: ") + be->strerror(rc));
	} else {
		walk_side_host(in, host);
		out.n_rec = (int64_t)host.rec.size(), out.rec = host.rec.data(), out.rep = host.rep.data(), out.cnt = host.cnt.data();
		out.n_gene = (int64_t)host.gene_seg.size(), out.gene_bub = host.gene_bub.data(), out.gene_seg = host.gene_seg.data(), out.gene_first = host.gene_first.data();
	}
	std::vector<std::pair<int64_t, int32_t>> gl;
	for (int64_t k0 = 0; k0 < out.n_gene;) {
		const int32_t b = out.gene_bub[k0];
		if (b < 0 || (size_t)b >= bb.size() || out.gene_seg[k0] < 0 || out.gene_seg[k0] >= g.n_seg()) throw CallError("call_bubbles: gene out of range");
		int64_t k1 = k0;
		gl.clear();
		for (; k1 < out.n_gene && out.gene_bub[k1] == b; ++k1) gl.emplace_back(out.gene_first[k1], out.gene_seg[k1]);
		std::sort(gl.begin(), gl.end());
		Bubble &x = bb[(size_t)b];
		x.n_gene = (int32_t)gl.size();
		for (auto &p : gl) x.gene.push_back(p.second);
		k0 = k1;
	}
	std::vector<int64_t> slot;
	for (int64_t r0 = 0; r0 < out.n_rec;) {
		const int32_t b = out.rec[r0].bo >> 1;
		int64_t r1 = r0;
		while (r1 < out.n_rec && out.rec[r1].bo >> 1 == b) ++r1;
		if (b < 0 || (size_t)b >= bb.size()) throw CallError("call_bubbles: record out of range");
		for (int64_t r = r0; r < r1; ++r) {
			const pga_call_rec_t &x = out.rec[r];
			if (x.walk < 0 || (size_t)x.walk >= g.walk_asm.size() || x.st_off < 0 || x.st_off >= x.en_off || g.walk_off[(size_t)x.walk] + x.en_off >= g.walk_off[(size_t)x.walk + 1])
				throw CallError("call_bubbles: record out of range");
		}
		Bubble &x = bb[(size_t)b];
		if (x.n_gene > max_ext) { x.gene.clear(); r0 = r1; continue; }
		slot.assign((size_t)(r1 - r0), -1);
		for (int64_t r = r0; r < r1; ++r) {
			const int64_t f = out.rep[r];
			if (f < r0 || f > r) throw CallError("call_bubbles: allele representative out of range");
			if (f == r) slot[(size_t)(r - r0)] = (int64_t)x.al.size(), x.al.push_back({out.cnt[r], r, {}});
			if (slot[(size_t)(f - r0)] < 0) throw CallError("call_bubbles: allele representative is not its own");
			x.al[(size_t)slot[(size_t)(f - r0)]].walks.push_back(out.rec[r].walk);
		}
		for (const auto &a : x.al) if ((int64_t)a.walks.size() != a.n) throw CallError("call_bubbles: allele count mismatch");
		std::stable_sort(x.al.begin(), x.al.end(), [](const Bubble::Allele &a, const Bubble::Allele &c) { return a.n > c.n; });
		r0 = r1;
	}
	// the path of every allele, from its first record
	for (Bubble &x : bb)
		for (auto &a : x.al) {
			const pga_call_rec_t &r = out.rec[a.rec];
			const int32_t *w = g.step.data() + g.walk_off[(size_t)r.walk];
			std::vector<int32_t> p;
			if ((r.bo & 1) == 0) for (int32_t k = r.st_off; k <= r.en_off; ++k) p.push_back(w[k]);
			else for (int32_t k = r.en_off; k >= r.st_off; --k) p.push_back(w[k] ^ 1);
			a.rec = -1;
			a.walks.insert(a.walks.begin(), (int32_t)p.size());
			a.walks.insert(a.walks.begin() + 1, p.begin(), p.end());
		}
}

// ---------------------------------------------------------------------------------------------------------------------------
// output
// ---------------------------------------------------------------------------------------------------------------------------
struct Out {
	std::string s;
	FILE *fp;
	explicit Out(FILE *f) : fp(f) {}
	Out &str(const std::string &x) { s += x; return *this; }
	Out &chr(char c) { s += c; return *this; }
	Out &num(int64_t v) { s += std::to_string(v); return *this; }
	void line() { s += '\n'; if (s.size() > (1u << 20)) flush(); }
	void flush() { std::fwrite(s.data(), 1, s.size(), fp); s.clear(); }
};

void side(Out &o, const Graph &g, int32_t v) { o.chr("><"[v & 1]).str(g.name[(size_t)(v >> 1)]); }

void print_report(Out &o, const Graph &g, const std::vector<Bubble> &bb)
{
	o.str("CC\tFB  bbID  parID  side1  side2").line();
	o.str("CC\tBB  bbID  parID  side1  side2  #alleles  #genes  geneList  supportingAsm").line();
	o.str("CC\tAL  #hap  walk").line();
	o.str("CC").line();
	for (size_t i = 0; i < bb.size(); ++i) {
		const Bubble &b = bb[i];
		auto head = [&](const char *tag) {
			o.str(tag).chr('\t').num((int64_t)i).chr('\t').num(b.par).chr('\t').num(b.cec).chr('\t');
			side(o, g, b.vs), o.chr('\t'), side(o, g, b.ve);
		};
		if (b.flt) { // with walks, a filtered bubble has (empty) allele lists too, and they close with "//"
			head("FB"), o.line();
			if (b.has_walks) o.str("//").line();
			continue;
		}
		if (b.has_walks) {
			if (b.al.size() < 2) continue;
			head("BB"), o.chr('\t').num((int64_t)b.al.size()).chr('\t');
			if (b.gene.empty()) o.num(b.n_gene);
			else {
				o.num((int64_t)b.gene.size()).chr('\t');
				for (size_t k = 0; k < b.gene.size(); ++k) { if (k) o.chr(','); o.str(g.name[(size_t)b.gene[k]]); }
			}
			o.line();
			for (const auto &a : b.al) { // walks = [path length, path..., walk ids...]
				const int32_t pl = a.walks[0];
				o.str("AL\t").num(a.n).chr('\t');
				for (int32_t k = 1; k <= pl; ++k) side(o, g, a.walks[(size_t)k]);
				o.chr('\t');
				for (size_t k = (size_t)pl + 1; k < a.walks.size(); ++k) { if (k > (size_t)pl + 1) o.chr(','); o.str(g.walk_asm[(size_t)a.walks[k]]); }
				o.line();
			}
			o.str("//").line();
		} else {
			head("BB"), o.str("\t-1\t").num((int64_t)b.seg.size()).chr('\t');
			for (size_t k = 0; k < b.seg.size(); ++k) { if (k) o.chr(','); o.str(g.name[(size_t)b.seg[k]]); }
			o.line();
		}
	}
}

void edge_label(Out &o, const Graph &g, const Net::Edge &a)
{
	o.num(a.v).chr(',').num(a.w).chr('\t');
	if (a.seg < g.n_seg()) o.chr(a.ori > 0 ? '>' : '<').str(g.name[(size_t)a.seg]);
	else o.chr('*');
}

double t_walk = 0.0; // wall seconds of the walk side of the last run_call

int run_call(Graph &g, const pg_call_opt_t *opt)
{
	pg_call_opt_t def;
	pg_call_opt_init(&def);
	const pg_call_opt_t &o = opt ? *opt : def;
	const int64_t max_ext = o.max_ext;
	try {
		Net net(g, o.add_super != 0, o.ref);
		std::vector<Bubble> bb;
		if (o.use_pst) {
			bb = net.pst();
			std::vector<int64_t> flag((size_t)g.n_vtx(), -1);
			for (size_t i = 0; i < bb.size(); ++i) {
				std::vector<int32_t> r = bubble_between(g, bb[i].vs, bb[i].ve, flag, (int64_t)i, max_ext);
				if (r.empty()) bb[i].flt = true;
				else bb[i].seg = std::move(r);
			}
		} else {
			net.mark_cec();
			bb = bubbles_by_bfs(g, max_ext);
		}
		const double t1 = now_sec();
		if (!o.ignore_walk && !g.walk_asm.empty()) walk_side(g, bb, max_ext);
		t_walk = now_sec() - t1;
		Out out(out_stream());
		if (o.print_dfs) {
			for (int32_t v : net.by_discovery())
				for (int64_t i = net.off[(size_t)v]; i < net.off[(size_t)v + 1]; ++i) {
					const Net::Edge &a = net.e[(size_t)i];
					if (a.type != 1 && a.type != 2) continue;
					out.str("DF\t").str(a.type == 1 ? "tree" : "back").chr('\t'), edge_label(out, g, a), out.line();
				}
		}
		if (o.print_bandage) {
			out.str("segment,label").line();
			for (const Net::Edge &a : net.e)
				if (a.seg < g.n_seg() && (a.type == 1 || a.type == 2) && a.cec >= 0) out.str(g.name[(size_t)a.seg]).chr(',').num(a.cec).line();
		}
		if (o.print_cec) {
			for (const Net::Edge &a : net.e) {
				if (a.type != 1 && a.type != 2) continue;
				out.str("EC\t").num(a.cec).chr('\t').str(a.type == 1 ? "tree" : "back").chr('\t'), edge_label(out, g, a), out.line();
			}
		}
		if (!o.print_dfs && !o.print_bandage && !o.print_cec) print_report(out, g, bb);
		out.flush();
		std::fflush(out.fp);
	} catch (const CallError &e) {
		std::fprintf(stderr, "Error: %s\n", e.what());
		return -2;
	}
	return 0;
}

// PANGENE_CALL_TIMING=1: one line on stderr per call (tests/run_call_timing.py reads it)
void report_time(const char *route, const Graph &g, double t_call, double t_collect = 0.0)
{
	if (std::getenv("PANGENE_CALL_TIMING") == nullptr) return;
	std::fprintf(stderr, "[call-timing] route=%s segments=%d walks=%zu steps=%zu collect_ms=%.3f call_ms=%.3f walk_side_ms=%.3f\n", route, g.n_seg(),
	             g.walk_asm.size(), g.step.size(), t_collect * 1e3, t_call * 1e3, t_walk * 1e3);
}

} // namespace

// The in-memory route: segments and links as pg_write_graph prints them, walks as pg_write_walk does (gfa_writer.cpp).
int walk_lists(pg_graph_t *q, std::vector<std::string> &asm_name, std::vector<int32_t> &step, std::vector<int64_t> &walk_off);

} // namespace pgx

using namespace pgx;

extern "C" {

void pg_call_opt_init(pg_call_opt_t *o)
{
	std::memset(o, 0, sizeof(*o));
	o->max_ext = 100;
}

int pg_call_file(const char *gfa_fn, const pg_call_opt_t *o)
{
	std::vector<std::string> lines;
	if (read_lines(gfa_fn, lines) != 0) { std::fprintf(stderr, "Error: cannot open %s\n", gfa_fn ? gfa_fn : "-"); return -1; }
	Graph g;
	parse_gfa(lines, g);
	lines.clear();
	const double t0 = now_sec();
	const int rc = run_call(g, o);
	report_time("file", g, now_sec() - t0);
	return rc;
}

void pg_write_call(pg_graph_t *q, const pg_call_opt_t *o)
{
	const double t0 = now_sec();
	const pg_data_t *d = q->d;
	Graph g;
	for (int32_t i = 0; i < q->n_seg; ++i) g.seg_add(d->gene[q->seg[i].gid].name);
	for (int32_t i = 0; i < q->n_arc; ++i) { // the written L-lines carry no SR:i tag
		const uint64_t x = q->arc[i].x;
		g.arc.push_back({(int32_t)(x >> 32), (int32_t)(uint32_t)x, false});
	}
	g.walk_off.clear();
	if (walk_lists(q, g.walk_asm, g.step, g.walk_off) != 0) return;
	g.index();
	const double t1 = now_sec();
	if (run_call(g, o) != 0) set_error(PGA_ERR_INVARIANT, "pg_write_call");
	report_time("memory", g, now_sec() - t1, t1 - t0);
}

} // extern "C"
