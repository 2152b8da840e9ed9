// Test support: sorts the same (key, index) arrays with the reference's radix sort (ksort_ref_stub.c) and with
// pangene_amd/csrc/host/ksort_exact.hpp and requires the same permutation -- the order-exact restatement claim of SURVEY 9.1.
// Built with -DKSORT_REF (linked with ksort_ref_stub.o): `ksort_check` compares the two directly, `ksort_check record FILE` writes a
// digest of the reference's permutation of every case to FILE.  Built without it: `ksort_check check FILE` compares ksort_exact's
// permutations with the digests recorded in FILE (tests/golden/ksort_reference_digests.txt).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ksort_exact.hpp"
struct t128_t { uint64_t x, y; };
#ifdef KSORT_REF
extern "C" void ref_radix_sort_128(t128_t *a, size_t n);
#endif
static uint64_t rng_state = 88172645463325252ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static uint64_t digest(const std::vector<t128_t> &a) // FNV-1a over the sorted (key, index) pairs
{
	uint64_t h = 14695981039346656037ull;
	for (const t128_t &e : a)
		for (uint64_t w : { e.x, e.y })
			for (int k = 0; k < 8; ++k) h = (h ^ ((w >> (8 * k)) & 0xff)) * 1099511628211ull;
	return h;
}
int main(int argc, char **argv)
{
	const char *mode = argc > 1 ? argv[1] : "live";
	FILE *fp = nullptr;
	if (std::strcmp(mode, "live") != 0) {
		if (argc < 3 || !(fp = std::fopen(argv[2], std::strcmp(mode, "record") == 0 ? "w" : "r"))) { std::printf("usage: ksort_check [record|check FILE]\n"); return 2; }
	}
#ifndef KSORT_REF
	if (std::strcmp(mode, "check") != 0) { std::printf("built without the reference's sort: only `check FILE`\n"); return 2; }
#endif
	long n_case = 0, n_bad = 0;
	const size_t sizes[] = { 1, 2, 63, 64, 65, 100, 257, 1000, 4097, 20000, 100003 };
	for (size_t n : sizes)
		for (int bits = 1; bits <= 40; bits += 3)        // few distinct keys ... many
			for (int rep = 0; rep < (n < 5000 ? 8 : 2); ++rep) {
				std::vector<t128_t> a(n), b;
				const uint64_t mask = bits >= 64 ? ~0ull : ((1ull << bits) - 1);
				const int shift = (int)(rnd() % 24);          // keys that only differ in higher bytes too
				for (size_t i = 0; i < n; ++i) a[i].x = (rnd() & mask) << shift, a[i].y = i;
				if (rep & 1) for (size_t i = 0; i < n; ++i) a[i].x = a[i].x / 300 * 300; // the 300-bp grid of the fuzz sets: long tie groups
				b = a;
				pgx::ksort_exact(b.data(), n, [](const t128_t &e) { return e.x; });
				++n_case;
				if (std::strcmp(mode, "check") == 0) {
					unsigned long long want = 0;
					if (std::fscanf(fp, "%llx", &want) != 1 || want != digest(b)) { ++n_bad; std::printf("MISMATCH n=%zu bits=%d rep=%d (digest)\n", n, bits, rep); }
					continue;
				}
#ifdef KSORT_REF
				ref_radix_sort_128(a.data(), n);
				if (fp) { std::fprintf(fp, "%016llx\n", (unsigned long long)digest(a)); continue; }
				for (size_t i = 0; i < n; ++i)
					if (a[i].x != b[i].x || a[i].y != b[i].y) { ++n_bad; std::printf("MISMATCH n=%zu bits=%d rep=%d at %zu\n", n, bits, rep, i); break; }
#endif
			}
	if (fp) std::fclose(fp);
	std::printf("ksort check: %ld cases, %ld mismatches\n", n_case, n_bad);
	return n_bad != 0;
}
