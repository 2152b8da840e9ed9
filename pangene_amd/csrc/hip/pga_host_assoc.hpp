// pga_pan_assoc (include/pangene_hip.h): the gene associations of pangene assoc on the device (k_assoc.hpp).  Context-free: it runs on
// a stream of its own on the current device.  The device buffers and the page-locked results are kept from call to call and only
// ever grow; pga_host_trim(0) gives them back.  The results wait in the page-locked buffers until the next call.
//
// The host reads two words back before the result: E, the number of eligible rows (it sizes the tile grid), and the number of
// selected pairs (it sizes the sort and the download).  When that number is above what the record buffers hold, they grow to it and
// the pairs kernel runs once more -- the count was exact, so once is enough.  PANGENE_ASSOC_CAP=n sets the capacity the first run
// starts from (default 1 048 576 records), so that tests reach the second run.

constexpr int32_t ASSOC_MAX_ASM = 16777215, ASSOC_MAX_GENE = 16777215;
constexpr int32_t ASSOC_MAX_ELIG = 4194304;            // 32 768 tile rows: 536 887 296 tiles, an int32 tile number
constexpr int64_t ASSOC_MAX_RECORDS = (int64_t)1 << 30; // the sort's positions are 32-bit
constexpr int64_t ASSOC_CAP0 = (int64_t)1 << 20;

struct AssocBuf {
	enum { BITS, COUNT, FLAG, MAP, TILE, SCAL, CBITS, CA, KEYS, KALT, VALS, VALT, TABLE, OUT, N_BUF };
	enum { H_PAIR, H_COUNT, H_SCAL, N_HOST }; // page-locked
};
static_assert(AssocBuf::N_BUF <= PAN_MAX_DEV && AssocBuf::N_HOST <= PAN_MAX_HOST, "the pool has room");

extern "C" int pga_pan_assoc(const pga_assoc_in_t *in, pga_assoc_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->n_pair = 0, out->pair = nullptr, out->count = nullptr;
	if (in == nullptr) return PGA_ERR_ARG;
	const int32_t G = in->n_gene, A = in->n_asm;
	if (G < 0 || A < 0 || in->min_count < 1 || in->r_permille < 0 || in->r_permille > 1000 || in->sign < 0 || in->sign > 2 || in->max_pair < 0) return PGA_ERR_ARG;
	if (A > ASSOC_MAX_ASM || G > ASSOC_MAX_GENE) return PGA_ERR_RANGE;
	const int32_t W = (A + 31) / 32;
	if (G > 0 && W > 0 && in->bits == nullptr) return PGA_ERR_ARG;
	PanDev &m = g_pan[PAN_ASSOC];
	std::lock_guard<std::mutex> lk(m.mu);
	int32_t *h_count = m.get_host<int32_t>(AssocBuf::H_COUNT, (size_t)G);
	int32_t *h_pair = m.get_host<int32_t>(AssocBuf::H_PAIR, 3);
	uint64_t *h_scal = m.get_host<uint64_t>(AssocBuf::H_SCAL, 2);
	PANMEM(h_count); PANMEM(h_pair); PANMEM(h_scal);
	out->count = h_count, out->pair = h_pair;
	if (G == 0) return 0;
	if (W == 0) { memset(h_count, 0, sizeof(int32_t) * (size_t)G); return 0; } // no assemblies: nothing is eligible
	hipStream_t st;
	PANCHK(m, m.stream(&st));

	// prepare: counts, eligibility, the places of the eligible rows
	const size_t n_word = (size_t)G * (size_t)W;
	uint32_t *d_bits = m.get<uint32_t>(AssocBuf::BITS, n_word);
	int32_t *d_count = m.get<int32_t>(AssocBuf::COUNT, (size_t)G), *d_flag = m.get<int32_t>(AssocBuf::FLAG, (size_t)G), *d_map = m.get<int32_t>(AssocBuf::MAP, (size_t)G);
	I32 *d_tile = m.get<I32>(AssocBuf::TILE, (size_t)std::max<int64_t>(scan_tiles(G), 256));
	uint64_t *d_scal = m.get<uint64_t>(AssocBuf::SCAL, 2); // [0] the pair counter, [1] E (its low word)
	PANMEM(d_bits); PANMEM(d_count); PANMEM(d_flag); PANMEM(d_map); PANMEM(d_tile); PANMEM(d_scal);
	PANCHK(m, hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * n_word, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_scal, 0, sizeof(uint64_t) * 2, st));
	const unsigned row_blocks = (unsigned)(((int64_t)G + BLOCK / ASSOC_ROW_LANES - 1) / (BLOCK / ASSOC_ROW_LANES));
	hipLaunchKernelGGL(k_assoc_count, dim3(row_blocks), dim3(BLOCK), 0, st, d_bits, G, W, A, in->min_count, d_count, d_flag);
	device_scan<I32, OpSum>(InI32{d_flag}, OutAssocMap{d_flag, d_map, (int32_t *)(d_scal + 1), (int64_t)G}, (int64_t)G, d_tile, OpSum{}, I32{0}, st);
	PANCHK(m, hipGetLastError());
	PANCHK(m, hipMemcpyAsync(h_count, d_count, sizeof(int32_t) * (size_t)G, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipMemcpyAsync(h_scal, d_scal, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	const int64_t E64 = (int64_t)(h_scal[1] & 0xffffffffu);
	if (E64 > ASSOC_MAX_ELIG) return PGA_ERR_RANGE;
	const int32_t E = (int32_t)E64;
	if (E < 2) return 0;

	// the eligible rows next to each other
	uint32_t *d_cbits = m.get<uint32_t>(AssocBuf::CBITS, (size_t)E * (size_t)W);
	int32_t *d_ca = m.get<int32_t>(AssocBuf::CA, (size_t)E);
	PANMEM(d_cbits); PANMEM(d_ca);
	const int64_t gather_blocks = std::min<int64_t>(((int64_t)E * W + BLOCK - 1) / BLOCK, (int64_t)1 << 20);
	hipLaunchKernelGGL(k_assoc_gather, dim3((unsigned)gather_blocks), dim3(BLOCK), 0, st, d_bits, d_map, d_count, E, W, d_cbits, d_ca);

	// pairs: the first run with the capacity at hand, a second one when more pairs passed than it holds
	const int64_t max_pair = std::min(in->max_pair, ASSOC_MAX_RECORDS);
	int64_t want = ASSOC_CAP0;
	if (const char *s = getenv("PANGENE_ASSOC_CAP")) { const long long v = atoll(s); if (v >= 1) want = std::min<int64_t>(v, ASSOC_MAX_RECORDS); }
	AssocPar par;
	par.E = E, par.W = W, par.n_chunk = (W + DIST_KC - 1) / DIST_KC, par.A = A, par.sign = in->sign;
	par.eb = 1;
	while (((int64_t)1 << par.eb) < E) ++par.eb;
	par.p2 = (uint32_t)in->r_permille * (uint32_t)in->r_permille, par.p2s = (double)par.p2 / 1e6;
	const int32_t T = (E + DIST_TILE - 1) / DIST_TILE, n_tile = (int32_t)((int64_t)T * (T + 1) / 2);
	int64_t total = 0;
	uint64_t *d_keys = nullptr;
	uint32_t *d_vals = nullptr;
	for (int run = 0; run < 2; ++run) {
		d_keys = m.get<uint64_t>(AssocBuf::KEYS, (size_t)want);
		d_vals = m.get<uint32_t>(AssocBuf::VALS, (size_t)want);
		PANMEM(d_keys); PANMEM(d_vals);
		par.cap = want;
		if (run) PANCHK(m, hipMemsetAsync(d_scal, 0, sizeof(uint64_t), st));
		hipLaunchKernelGGL(k_assoc_pairs, dim3((unsigned)n_tile), dim3(BLOCK), 0, st, d_cbits, d_ca, par, (unsigned long long *)d_scal, d_keys, d_vals);
		PANCHK(m, hipGetLastError());
		PANCHK(m, hipMemcpyAsync(h_scal, d_scal, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
		PANCHK(m, hipStreamSynchronize(st));
		total = (int64_t)h_scal[0];
		out->n_pair = total;
		if (total > max_pair) { out->pair = nullptr; return PGA_ERR_RANGE; }
		if (total <= want) break;
		want = total;
	}
	if (total == 0) return 0;

	// ascending (g, h): the places keep the order of the rows, so the keys sort as the pairs do
	RadixBufs rb;
	rb.k_alt = m.get<uint64_t>(AssocBuf::KALT, (size_t)total);
	rb.v_alt = m.get<uint32_t>(AssocBuf::VALT, (size_t)total);
	rb.table = m.get<uint32_t>(AssocBuf::TABLE, (size_t)rs_table_len(total));
	rb.tile_buf = (int32_t *)d_tile;
	int32_t *d_out = m.get<int32_t>(AssocBuf::OUT, (size_t)total * 3);
	h_pair = m.get_host<int32_t>(AssocBuf::H_PAIR, (size_t)total * 3);
	PANMEM(rb.k_alt); PANMEM(rb.v_alt); PANMEM(rb.table); PANMEM(d_out); PANMEM(h_pair);
	out->pair = h_pair;
	uint64_t *k_res;
	uint32_t *v_res;
	device_radix_sort(d_keys, d_vals, total, 2 * par.eb, rb, &k_res, &v_res, st);
	hipLaunchKernelGGL(k_assoc_emit, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, k_res, v_res, total, par.eb, d_map, d_out);
	PANCHK(m, hipGetLastError());
	PANCHK(m, hipMemcpyAsync(h_pair, d_out, sizeof(int32_t) * 3 * (size_t)total, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	return 0;
}
