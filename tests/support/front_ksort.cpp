// Test support: the order pangene_amd/csrc/host/ksort_exact.hpp (the replay of the reference's unstable radix sort) gives (key, index)
// pairs, for tests/test_front.py.  `front_ksort IN OUT`: IN holds n little-endian uint64 keys, OUT receives the n indices as int32, in
// sorted order.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "ksort_exact.hpp"
struct t128_t { uint64_t x, y; };
int main(int argc, char **argv)
{
	if (argc != 3) return 2;
	std::FILE *fi = std::fopen(argv[1], "rb");
	if (!fi) return 2;
	std::vector<t128_t> a;
	uint64_t k;
	while (std::fread(&k, sizeof(k), 1, fi) == 1) a.push_back(t128_t{k, (uint64_t)a.size()});
	std::fclose(fi);
	pgx::ksort_exact(a.data(), a.size(), [](const t128_t &e) { return e.x; });
	std::FILE *fo = std::fopen(argv[2], "wb");
	if (!fo) return 2;
	for (const t128_t &e : a) { const int32_t i = (int32_t)e.y; std::fwrite(&i, sizeof(i), 1, fo); }
	std::fclose(fo);
	return 0;
}
