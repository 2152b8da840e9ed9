// pan_common.hpp -- what the pan commands (curves.cpp, dist.cpp, assoc.cpp, trait.cpp, tree.cpp) share on the host: packing a matrix
// into bit rows, the random orders, Benjamini-Hochberg q values, the buffered writer of their tables.  Included at the end of pg_internal.hpp.
#pragma once
#include <algorithm>
#include <numeric>
#include <vector>

namespace pgx {

inline uint64_t mix64(uint64_t z) // splitmix64's output function
{
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

// order p >= 1 of A columns: Fisher-Yates from the last column down, j = next() % (i + 1).  The goldens pin the sequence.
inline void fisher_yates_order(int32_t A, uint32_t seed, uint32_t p, int32_t *o)
{
	for (int32_t i = 0; i < A; ++i) o[i] = i;
	uint64_t x = mix64((uint64_t)seed << 32 | (uint64_t)p);
	for (int32_t i = A - 1; i >= 1; --i) {
		x += 0x9E3779B97F4A7C15ull;
		const uint64_t j = mix64(x) % (uint64_t)(i + 1);
		std::swap(o[i], o[j]);
	}
}

// an entry that counts as present: a presence byte that is not zero, a gfa2matrix occurrence count above zero
inline bool pan_present(uint8_t v) { return v != 0; }
inline bool pan_present(int32_t v) { return v > 0; }

// src[R][C], row-major -> bits[R][(C + 31) / 32]: bit c of row r
template <class T> void pack_rows(const T *src, int32_t R, int32_t C, std::vector<uint32_t> &bits)
{
	const size_t W = ((size_t)C + 31) / 32;
	bits.assign((size_t)R * W, 0);
	for (int32_t r = 0; r < R; ++r) {
		const T *row = src + (size_t)r * C;
		uint32_t *b = bits.data() + (size_t)r * W;
		for (int32_t c = 0; c < C; ++c)
			if (pan_present(row[c])) b[c >> 5] |= 1u << (c & 31);
	}
}

// the same transposed: src[R][C] -> bits[C][(R + 31) / 32]: bit r of row c
template <class T> void pack_cols(const T *src, int32_t R, int32_t C, std::vector<uint32_t> &bits)
{
	const size_t W = ((size_t)R + 31) / 32;
	bits.assign((size_t)C * W, 0);
	for (int32_t r = 0; r < R; ++r) {
		const T *row = src + (size_t)r * C;
		const uint32_t bit = 1u << (r & 31);
		uint32_t *col = bits.data() + (size_t)(r >> 5);
		for (int32_t c = 0; c < C; ++c)
			if (pan_present(row[c])) col[(size_t)c * W] |= bit;
	}
}

// a table on its way to out_stream(): text is collected and written whenever 1 MiB is there; finish() writes the rest and flushes
struct OutBuf {
	std::string s;
	void flush_if_full() { if (s.size() >= (1u << 20)) std::fwrite(s.data(), 1, s.size(), out_stream()), s.clear(); }
	void finish() { std::fwrite(s.data(), 1, s.size(), out_stream()), s.clear(); std::fflush(out_stream()); }
};

// Benjamini-Hochberg q of p (in row order): sorted ascending, ties by row; q_(i) = min over j >= i of p_(j) m / j, capped at 1
inline void bh_q(const std::vector<double> &p, std::vector<double> &q)
{
	const size_t m = p.size();
	q.assign(m, 0.0);
	std::vector<size_t> idx(m);
	std::iota(idx.begin(), idx.end(), (size_t)0);
	std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return p[x] < p[y]; }); // ties by row
	double run = 1.0;
	for (size_t j = m; j >= 1; --j) {
		run = std::min(run, p[idx[j - 1]] * (double)m / (double)j);
		q[idx[j - 1]] = run;
	}
}

inline int cannot_open(const char *fn) { std::fprintf(stderr, "Error: cannot open %s\n", fn ? fn : "-"); return -1; }

} // namespace pgx
