// pga_pan_coevo (include/pangene_hip.h): co-evolution of the items on a tree on the device (k_coevo.hpp over k_gainloss.hpp).  Context-free:
// it runs on a stream of its own on the current device.  The device buffers and the page-locked staging and result memory are kept from
// call to call in the PAN_COEVO pool and only ever grow; pga_host_trim(0) gives them back.  The results wait in the page-locked buffers
// until the next call.
//
// The host checks the program as pga_pan_gainloss does and uploads it with par and all the bit rows.  The items go through k_gl_up and
// k_gl_down in chunks (pga_coevo_chunk); then k_ce_flag and a scan over all items give the events, the flags and the places.  The host
// waits three times: for E, the number of eligible items (it sizes the row buffer and the tile grid), for the number of selected pairs
// (it sizes the sort and the download; above the capacity the record buffers grow to it and k_ce_pairs runs once more -- the count was
// exact, so once is enough) and for the result.  k_ce_rows needs a chunk's state rows and the places of its items; the places are known
// only after every chunk has been reconstructed, so with one chunk -- the rule below makes that the common case -- the rows are made
// from the state rows still in place, and with several chunks each chunk is reconstructed once more before its rows are made.
constexpr int32_t COEVO_MAX_ELIG = 4194304;            // 32 768 tile rows: an int32 tile number
constexpr int64_t COEVO_MAX_RECORDS = (int64_t)1 << 30; // the sort's positions are 32-bit
constexpr int64_t COEVO_CAP0 = (int64_t)1 << 20;

struct CoevoBuf {
	enum { OPS, PAR, BITS, K0, K1, ST, GENE, EVENTS, FLAG, MAP, PLACE, TILE, SCAL, ROWS, CE, KEYS, KALT, VALS, VALT, SO, TABLE, OUT, N_BUF };
	enum { H_IN, H_EVENTS, H_PAIR, N_HOST }; // page-locked: two scalars, then the packed program and par; the results
};
static_assert(CoevoBuf::N_BUF <= PAN_MAX_DEV && CoevoBuf::N_HOST <= PAN_MAX_HOST, "the pool has no room for the co-evolution buffers");

// items per chunk over a tree of n_leaf leaves: PANGENE_COEVO_CHUNK (rounded up to a multiple of 1 024), or pga_gainloss_chunk's rule
extern "C" int32_t pga_coevo_chunk(int32_t n_leaf)
{
	const int64_t c = pan_env("PANGENE_COEVO_CHUNK", 0, (int64_t)1 << 24);
	return c > 0 ? (int32_t)((c + 1023) / 1024 * 1024) : pga_gainloss_chunk(n_leaf);
}

extern "C" int pga_pan_coevo(const pga_coevo_in_t *in, pga_coevo_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->events = nullptr, out->n_pair = 0, out->pair = nullptr;
	if (in == nullptr) return PGA_ERR_ARG;
	const int32_t G = in->n_gene, L = in->n_leaf;
	if (G < 0 || L < 0) return PGA_ERR_ARG;
	if (L > GL_MAX_LEAF || G > GL_MAX_GENE) return PGA_ERR_RANGE;
	if (in->gain < 1 || in->gain > 255 || in->loss < 1 || in->loss > 255) return PGA_ERR_RANGE;
	if (in->mode != 0 && in->mode != 1) return PGA_ERR_ARG;
	if (in->min_events < 1 || in->r_permille < 0 || in->r_permille > 1000 || in->sign < 0 || in->sign > 2 || in->max_pair < 0) return PGA_ERR_ARG;
	if (in->ev_rows != nullptr && in->ev_cap < 0) return PGA_ERR_ARG;
	const int32_t W = (G + 31) / 32, n_op = L > 0 ? 2 * L - 1 : 0, OW = (n_op + 31) / 32;
	if (L > 0 && (in->op == nullptr || in->par == nullptr || (G > 0 && in->bits == nullptr))) return PGA_ERR_ARG;
	// the program: n_leaf pushes, no join of fewer than two entries, one entry left; the depth it needs; par names the join that takes a node
	int32_t depth = 0, pushed = 0;
	std::vector<int32_t> made; // the ops whose nodes are on the stack
	for (int32_t k = 0; k < n_op; ++k) {
		if (in->op[k] == 0) ++pushed, made.push_back(k), depth = std::max(depth, (int32_t)made.size());
		else if (in->op[k] == 1 && made.size() >= 2) {
			if (in->par[made.back()] != k || in->par[made[made.size() - 2]] != k) return PGA_ERR_ARG;
			made.pop_back(), made.back() = k;
		} else return PGA_ERR_ARG;
	}
	if (n_op > 0 && (made.size() != 1 || pushed != L || in->par[n_op - 1] != -1)) return PGA_ERR_ARG;
	if (depth > GL_DEPTH) return PGA_ERR_RANGE;
	PanDev &m = g_pan[PAN_COEVO];
	std::lock_guard<std::mutex> lk(m.mu);
	int32_t *h_events = m.get_host<int32_t>(CoevoBuf::H_EVENTS, (size_t)G);
	int32_t *h_pair = m.get_host<int32_t>(CoevoBuf::H_PAIR, 4);
	PANMEM(h_events); PANMEM(h_pair);
	out->events = h_events, out->pair = h_pair;
	memset(h_events, 0, sizeof(int32_t) * (size_t)G);
	if (G == 0 || L < 2) return 0; // no item or no branch: no launch
	const size_t n_scal = 4; // words of h_in before the program: [0, 1] the pair counter, [2] E
	uint32_t *h_in = m.get_host<uint32_t>(CoevoBuf::H_IN, n_scal + (size_t)OW + (size_t)n_op);
	PANMEM(h_in);
	uint64_t *h_scal = (uint64_t *)h_in;
	uint32_t *h_ops = h_in + n_scal;
	memset(h_ops, 0, sizeof(uint32_t) * (size_t)OW);
	for (int32_t k = 0; k < n_op; ++k) h_ops[k >> 5] |= (uint32_t)in->op[k] << (k & 31);
	memcpy(h_ops + OW, in->par, sizeof(int32_t) * (size_t)n_op);
	const int32_t chunk = pga_coevo_chunk(L);
	const int32_t WW = (std::min(chunk, G) + WAVE - 1) / WAVE; // 64-bit words of a row of the largest chunk
	const int32_t B = n_op - 1, WB = (B + 31) / 32;
	const size_t n_row = (size_t)n_op * (size_t)WW, n_word = (size_t)L * (size_t)W, n_gene4 = (size_t)G * 4;
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	uint32_t *d_ops = m.get<uint32_t>(CoevoBuf::OPS, (size_t)OW), *d_bits = m.get<uint32_t>(CoevoBuf::BITS, n_word);
	int32_t *d_par = m.get<int32_t>(CoevoBuf::PAR, (size_t)n_op), *d_gene = m.get<int32_t>(CoevoBuf::GENE, n_gene4);
	unsigned long long *d_k0 = m.get<unsigned long long>(CoevoBuf::K0, n_row), *d_k1 = m.get<unsigned long long>(CoevoBuf::K1, n_row);
	unsigned long long *d_st = m.get<unsigned long long>(CoevoBuf::ST, n_row);
	int32_t *d_events = m.get<int32_t>(CoevoBuf::EVENTS, (size_t)G), *d_flag = m.get<int32_t>(CoevoBuf::FLAG, (size_t)G);
	int32_t *d_map = m.get<int32_t>(CoevoBuf::MAP, (size_t)G), *d_place = m.get<int32_t>(CoevoBuf::PLACE, (size_t)G);
	I32 *d_tile = m.get<I32>(CoevoBuf::TILE, (size_t)std::max<int64_t>(scan_tiles(G), 256));
	uint64_t *d_scal = m.get<uint64_t>(CoevoBuf::SCAL, 2); // [0] the pair counter, [1] E (its low word)
	PANMEM(d_ops); PANMEM(d_bits); PANMEM(d_par); PANMEM(d_gene); PANMEM(d_k0); PANMEM(d_k1); PANMEM(d_st);
	PANMEM(d_events); PANMEM(d_flag); PANMEM(d_map); PANMEM(d_place); PANMEM(d_tile); PANMEM(d_scal);
	PANCHK(m, hipMemcpyAsync(d_ops, h_ops, sizeof(uint32_t) * (size_t)OW, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_par, h_ops + OW, sizeof(int32_t) * (size_t)n_op, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * n_word, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_scal, 0, sizeof(uint64_t) * 2, st));
	const size_t lds = sizeof(int32_t) * 2 * GL_BLOCK * (size_t)std::max(depth - 1, 1);
	auto reconstruct = [&](int32_t g0, int32_t Gc, int32_t WC) { // the chunk's rows are WC words long
		const unsigned blocks = (unsigned)((Gc + GL_BLOCK - 1) / GL_BLOCK);
		hipLaunchKernelGGL(k_gl_up, dim3(blocks), dim3(GL_BLOCK), lds, st, d_ops, d_bits, g0, Gc, W, L, n_op, in->gain, in->loss, in->mode, WC, d_k0, d_k1, d_gene);
		hipLaunchKernelGGL(k_gl_down, dim3(blocks), dim3(GL_BLOCK), 0, st, d_ops, g0, Gc, n_op, WC, d_k0, d_k1, d_st, d_gene);
	};
	for (int32_t g0 = 0; g0 < G; g0 += chunk) {
		const int32_t Gc = std::min(chunk, G - g0);
		reconstruct(g0, Gc, (Gc + WAVE - 1) / WAVE);
	}
	hipLaunchKernelGGL(k_ce_flag, dim3((unsigned)((G + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, d_gene, G, in->min_events, d_events, d_flag);
	device_scan<I32, OpSum>(InI32{d_flag}, OutCoevoMap{d_flag, d_map, d_place, (int32_t *)(d_scal + 1), (int64_t)G}, (int64_t)G, d_tile, OpSum{}, I32{0}, st);
	PANCHK(m, hipGetLastError());
	PANCHK(m, hipMemcpyAsync(h_events, d_events, sizeof(int32_t) * (size_t)G, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipMemcpyAsync(h_scal, d_scal, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	const int64_t E64 = (int64_t)(h_scal[1] & 0xffffffffu);
	if (E64 > COEVO_MAX_ELIG) return PGA_ERR_RANGE;
	const int32_t E = (int32_t)E64;
	if (E == 0 || (E < 2 && in->ev_rows == nullptr)) return 0;

	// the event rows of the eligible items, chunk by chunk
	const size_t n_ev = (size_t)E * 2 * (size_t)WB;
	uint32_t *d_rows = m.get<uint32_t>(CoevoBuf::ROWS, n_ev);
	int32_t *d_ce = m.get<int32_t>(CoevoBuf::CE, (size_t)E);
	PANMEM(d_rows); PANMEM(d_ce);
	hipLaunchKernelGGL(k_ce_gather, dim3((unsigned)((E + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, d_events, d_map, E, d_ce);
	for (int32_t g0 = 0; g0 < G; g0 += chunk) {
		const int32_t Gc = std::min(chunk, G - g0), WC = (Gc + WAVE - 1) / WAVE;
		if (G > chunk) reconstruct(g0, Gc, WC); // several chunks: this one's state rows again
		hipLaunchKernelGGL(k_ce_rows, dim3((unsigned)WC, (unsigned)((B + CE_SPAN - 1) / CE_SPAN)), dim3(BLOCK), 0, st, d_st, d_par, d_place, g0, Gc, B, WC, WB, d_rows);
	}
	PANCHK(m, hipGetLastError());
	if (in->ev_rows != nullptr) { // tests only: the first rows
		const size_t n_take = (size_t)std::min<int64_t>(E, in->ev_cap) * 2 * (size_t)WB;
		if (n_take > 0) PANCHK(m, hipMemcpyAsync(in->ev_rows, d_rows, sizeof(uint32_t) * n_take, hipMemcpyDeviceToHost, st));
		PANCHK(m, hipStreamSynchronize(st));
	}
	if (E < 2) return 0;

	// pairs: the first run with the capacity at hand, a second one when more pairs passed than it holds
	const int64_t max_pair = std::min(in->max_pair, COEVO_MAX_RECORDS);
	int64_t want = pan_env("PANGENE_COEVO_CAP", COEVO_CAP0, COEVO_MAX_RECORDS);
	CoevoPar par;
	par.E = E, par.WB = WB, par.n_chunk = (WB + DIST_KC - 1) / DIST_KC, par.sign = in->sign;
	par.eb = 1;
	while (((int64_t)1 << par.eb) < E) ++par.eb;
	par.p2 = (uint32_t)in->r_permille * (uint32_t)in->r_permille;
	const int32_t T = (E + DIST_TILE - 1) / DIST_TILE, n_tile = (int32_t)((int64_t)T * (T + 1) / 2);
	int64_t total = 0;
	uint64_t *d_keys = nullptr;
	uint32_t *d_vals = nullptr;
	uint2 *d_so = nullptr;
	for (int run = 0; run < 2; ++run) {
		d_keys = m.get<uint64_t>(CoevoBuf::KEYS, (size_t)want);
		d_vals = m.get<uint32_t>(CoevoBuf::VALS, (size_t)want);
		d_so = m.get<uint2>(CoevoBuf::SO, (size_t)want);
		PANMEM(d_keys); PANMEM(d_vals); PANMEM(d_so);
		par.cap = want;
		if (run) PANCHK(m, hipMemsetAsync(d_scal, 0, sizeof(uint64_t), st));
		hipLaunchKernelGGL(k_ce_pairs, dim3((unsigned)n_tile), dim3(BLOCK), 0, st, d_rows, d_ce, par, (unsigned long long *)d_scal, d_keys, d_vals, d_so);
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

	// ascending (i, j): the places keep the order of the items, so the keys sort as the pairs do
	RadixBufs rb;
	rb.k_alt = m.get<uint64_t>(CoevoBuf::KALT, (size_t)total);
	rb.v_alt = m.get<uint32_t>(CoevoBuf::VALT, (size_t)total);
	rb.table = m.get<uint32_t>(CoevoBuf::TABLE, (size_t)rs_table_len(total));
	rb.tile_buf = (int32_t *)d_tile;
	int32_t *d_out = m.get<int32_t>(CoevoBuf::OUT, (size_t)total * 4);
	h_pair = m.get_host<int32_t>(CoevoBuf::H_PAIR, (size_t)total * 4);
	PANMEM(rb.k_alt); PANMEM(rb.v_alt); PANMEM(rb.table); PANMEM(d_out); PANMEM(h_pair);
	out->pair = h_pair;
	uint64_t *k_res;
	uint32_t *v_res;
	device_radix_sort(d_keys, d_vals, total, 2 * par.eb, rb, &k_res, &v_res, st);
	hipLaunchKernelGGL(k_ce_emit, dim3((unsigned)((total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, k_res, v_res, d_so, total, par.eb, d_map, d_out);
	PANCHK(m, hipGetLastError());
	PANCHK(m, hipMemcpyAsync(h_pair, d_out, sizeof(int32_t) * 4 * (size_t)total, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	return 0;
}
