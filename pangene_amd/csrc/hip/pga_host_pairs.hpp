// pga_pan_pairs (include/pangene_hip.h): the tree dynamic programmes of pangene trait -L on the device (k_pairs.hpp).  Context-free: it
// runs on a stream of its own on the current device.  The device buffers and the page-locked staging and result memory are kept from call
// to call and only ever grow; pga_host_trim(0) gives them back.  The results wait in the page-locked buffer until the next call.
//
// The host checks the program (a malformed one would index the stack out of bounds) and finds the depth it needs, packs the program and
// the label rows into bit words, uploads, launches k_pairs -- one launch per 65 535 label rows -- and waits once.

struct PairsBuf {
	enum { OPS, BITS, HAS, ONE, OUT, N_BUF };
	enum { H_IN, H_OUT }; // page-locked: the packed program and label planes; the results
};

extern "C" int pga_pan_pairs(const pga_pairs_in_t *in, pga_pairs_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->out = nullptr;
	if (in == nullptr) return PGA_ERR_ARG;
	const int32_t G = in->n_gene, L = in->n_leaf, R = in->n_row;
	if (G < 0 || L < 0 || R < 0) return PGA_ERR_ARG;
	if (L > PAIRS_MAX_LEAF || G > PAIRS_MAX_GENE) return PGA_ERR_RANGE;
	const int32_t W = (G + 31) / 32, LW = (L + 31) / 32, n_op = L > 0 ? 2 * L - 1 : 0, OW = (n_op + 31) / 32;
	if (L > 0 && (in->op == nullptr || (G > 0 && in->bits == nullptr) || (R > 0 && in->label == nullptr))) return PGA_ERR_ARG;
	// the program: n_leaf pushes, no join of fewer than two entries, one entry left; the depth it needs
	int32_t depth = 0, sp = 0, pushed = 0;
	for (int32_t k = 0; k < n_op; ++k) {
		if (in->op[k] == 0) ++sp, ++pushed, depth = std::max(depth, sp);
		else if (in->op[k] == 1 && sp >= 2) --sp;
		else return PGA_ERR_ARG;
	}
	if (n_op > 0 && (sp != 1 || pushed != L)) return PGA_ERR_ARG;
	if (depth > PAIRS_DEPTH) return PGA_ERR_RANGE;
	PanDev &m = g_pan[PAN_PAIRS];
	std::lock_guard<std::mutex> lk(m.mu);
	const size_t n_out = (size_t)R * (size_t)G * 3;
	int32_t *h_out = m.get_host<int32_t>(PairsBuf::H_OUT, n_out);
	PANMEM(h_out);
	out->out = h_out;
	if (n_out == 0) return 0;
	if (L == 0) { memset(h_out, 0, sizeof(int32_t) * n_out); return 0; } // no leaves: no pairs
	const size_t n_plane = (size_t)R * (size_t)LW;
	uint32_t *h_in = m.get_host<uint32_t>(PairsBuf::H_IN, (size_t)OW + 2 * n_plane);
	PANMEM(h_in);
	uint32_t *h_ops = h_in, *h_has = h_in + OW, *h_one = h_has + n_plane;
	memset(h_in, 0, sizeof(uint32_t) * ((size_t)OW + 2 * n_plane));
	for (int32_t k = 0; k < n_op; ++k) h_ops[k >> 5] |= (uint32_t)in->op[k] << (k & 31);
	for (int32_t r = 0; r < R; ++r) {
		const int8_t *lab = in->label + (size_t)r * (size_t)L;
		for (int32_t x = 0; x < L; ++x) {
			if (lab[x] >= 0) h_has[(size_t)r * LW + (size_t)(x >> 5)] |= 1u << (x & 31);
			if (lab[x] > 0) h_one[(size_t)r * LW + (size_t)(x >> 5)] |= 1u << (x & 31);
		}
	}
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	const size_t n_word = (size_t)L * (size_t)W;
	uint32_t *d_ops = m.get<uint32_t>(PairsBuf::OPS, (size_t)OW), *d_bits = m.get<uint32_t>(PairsBuf::BITS, n_word);
	uint32_t *d_has = m.get<uint32_t>(PairsBuf::HAS, n_plane), *d_one = m.get<uint32_t>(PairsBuf::ONE, n_plane);
	int32_t *d_out = m.get<int32_t>(PairsBuf::OUT, n_out);
	PANMEM(d_ops); PANMEM(d_bits); PANMEM(d_has); PANMEM(d_one); PANMEM(d_out);
	PANCHK(m, hipMemcpyAsync(d_ops, h_ops, sizeof(uint32_t) * (size_t)OW, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_has, h_has, sizeof(uint32_t) * n_plane, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_one, h_one, sizeof(uint32_t) * n_plane, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * n_word, hipMemcpyHostToDevice, st));
	const unsigned gene_blocks = (unsigned)((G + PAIRS_BLOCK - 1) / PAIRS_BLOCK);
	const size_t lds = sizeof(int32_t) * 5 * PAIRS_BLOCK * (size_t)std::max(depth - 1, 1);
	for (int32_t r0 = 0; r0 < R; r0 += 65535) {
		const unsigned rows = (unsigned)std::min(65535, R - r0);
		hipLaunchKernelGGL(k_pairs, dim3(gene_blocks, rows, 2), dim3(PAIRS_BLOCK), lds, st, d_ops, d_bits, d_has, d_one, G, W, L, LW, n_op, r0, d_out);
		PANCHK(m, hipGetLastError());
	}
	PANCHK(m, hipMemcpyAsync(h_out, d_out, sizeof(int32_t) * n_out, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	return 0;
}
