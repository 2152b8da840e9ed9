// pga_pan_gainloss (include/pangene_hip.h): gene gain and loss on a tree on the device (k_gainloss.hpp).  Context-free: it runs on a
// stream of its own on the current device.  The device buffers and the page-locked staging and result memory are kept from call to call
// in the PAN_GAINLOSS pool and only ever grow; pga_host_trim(0) gives them back.  The results wait in the page-locked buffers until the
// next call.
//
// The host checks the program (a malformed one would index the stack out of bounds), finds the depth it needs and checks par against it,
// packs the program into bit words and uploads it with par and ALL the bit rows.  The items then go through in chunks, so that the three
// row arrays k0, k1 and st -- one bit per item and node each -- stay bounded: per chunk k_gl_up, k_gl_down and k_gl_node follow each other
// on the one stream, and k_gl_node adds the chunk's node totals into node.  Nothing is read back between the chunks and the host waits
// once, at the end (tests that ask for st_rows wait once more, after the first chunk).
constexpr int64_t GL_ROW_BYTES = (int64_t)1 << 30; // what k0, k1 and st of one chunk may take together

struct GainlossBuf {
	enum { OPS, PAR, BITS, K0, K1, ST, GENE, NODE, N_BUF };
	enum { H_IN, H_GENE, H_NODE }; // page-locked: the packed program and par; the results
};
static_assert(GainlossBuf::N_BUF <= PAN_MAX_DEV, "the pool has no room for the gain and loss buffers");

// items per chunk over a tree of n_leaf leaves: PANGENE_GAINLOSS_CHUNK (rounded up to a multiple of 1 024), or the largest multiple of
// 1 024 whose 3 (2 n_leaf - 1) bits per item fit GL_ROW_BYTES; never less than 1 024
extern "C" int32_t pga_gainloss_chunk(int32_t n_leaf)
{
	const int64_t n_op = std::max<int64_t>(2 * (int64_t)n_leaf - 1, 1);
	const int64_t fit = std::min<int64_t>(GL_ROW_BYTES * 8 / (3 * n_op), (int64_t)1 << 24) / 1024 * 1024;
	const int64_t c = pan_env("PANGENE_GAINLOSS_CHUNK", std::max<int64_t>(fit, 1024), (int64_t)1 << 24);
	return (int32_t)((c + 1023) / 1024 * 1024);
}

extern "C" int pga_pan_gainloss(const pga_gainloss_in_t *in, pga_gainloss_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->gene = nullptr, out->node = nullptr;
	if (in == nullptr) return PGA_ERR_ARG;
	const int32_t G = in->n_gene, L = in->n_leaf;
	if (G < 0 || L < 0) return PGA_ERR_ARG;
	if (L > GL_MAX_LEAF || G > GL_MAX_GENE) return PGA_ERR_RANGE;
	if (in->gain < 1 || in->gain > 255 || in->loss < 1 || in->loss > 255) return PGA_ERR_RANGE;
	if (in->mode != 0 && in->mode != 1) return PGA_ERR_ARG;
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
	PanDev &m = g_pan[PAN_GAINLOSS];
	std::lock_guard<std::mutex> lk(m.mu);
	const size_t n_gene4 = (size_t)G * 4, n_node3 = (size_t)n_op * 3;
	int32_t *h_gene = m.get_host<int32_t>(GainlossBuf::H_GENE, n_gene4);
	int64_t *h_node = m.get_host<int64_t>(GainlossBuf::H_NODE, n_node3);
	PANMEM(h_gene); PANMEM(h_node);
	out->gene = h_gene, out->node = h_node;
	memset(h_gene, 0, sizeof(int32_t) * n_gene4);
	memset(h_node, 0, sizeof(int64_t) * n_node3);
	if (G == 0 || L == 0) return 0; // nothing to reconstruct: no launch
	uint32_t *h_in = m.get_host<uint32_t>(GainlossBuf::H_IN, (size_t)OW + (size_t)n_op);
	PANMEM(h_in);
	memset(h_in, 0, sizeof(uint32_t) * (size_t)OW);
	for (int32_t k = 0; k < n_op; ++k) h_in[k >> 5] |= (uint32_t)in->op[k] << (k & 31);
	memcpy(h_in + OW, in->par, sizeof(int32_t) * (size_t)n_op);
	const int32_t chunk = pga_gainloss_chunk(L);
	const int32_t WW = (std::min(chunk, G) + WAVE - 1) / WAVE; // 64-bit words of a row of the largest chunk
	const size_t n_row = (size_t)n_op * (size_t)WW, n_word = (size_t)L * (size_t)W;
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	uint32_t *d_ops = m.get<uint32_t>(GainlossBuf::OPS, (size_t)OW), *d_bits = m.get<uint32_t>(GainlossBuf::BITS, n_word);
	int32_t *d_par = m.get<int32_t>(GainlossBuf::PAR, (size_t)n_op), *d_gene = m.get<int32_t>(GainlossBuf::GENE, n_gene4);
	unsigned long long *d_k0 = m.get<unsigned long long>(GainlossBuf::K0, n_row), *d_k1 = m.get<unsigned long long>(GainlossBuf::K1, n_row);
	unsigned long long *d_st = m.get<unsigned long long>(GainlossBuf::ST, n_row);
	long long *d_node = m.get<long long>(GainlossBuf::NODE, n_node3);
	PANMEM(d_ops); PANMEM(d_bits); PANMEM(d_par); PANMEM(d_gene); PANMEM(d_k0); PANMEM(d_k1); PANMEM(d_st); PANMEM(d_node);
	PANCHK(m, hipMemcpyAsync(d_ops, h_in, sizeof(uint32_t) * (size_t)OW, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_par, h_in + OW, sizeof(int32_t) * (size_t)n_op, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * n_word, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_node, 0, sizeof(long long) * n_node3, st));
	const size_t lds = sizeof(int32_t) * 2 * GL_BLOCK * (size_t)std::max(depth - 1, 1);
	for (int32_t g0 = 0; g0 < G; g0 += chunk) {
		const int32_t Gc = std::min(chunk, G - g0);
		const int32_t WC = (Gc + WAVE - 1) / WAVE; // the chunk's rows are WC words long: a shorter last chunk leaves no stale word in them
		const unsigned blocks = (unsigned)((Gc + GL_BLOCK - 1) / GL_BLOCK);
		hipLaunchKernelGGL(k_gl_up, dim3(blocks), dim3(GL_BLOCK), lds, st, d_ops, d_bits, g0, Gc, W, L, n_op, in->gain, in->loss, in->mode, WC, d_k0, d_k1, d_gene);
		hipLaunchKernelGGL(k_gl_down, dim3(blocks), dim3(GL_BLOCK), 0, st, d_ops, g0, Gc, n_op, WC, d_k0, d_k1, d_st, d_gene);
		hipLaunchKernelGGL(k_gl_node, dim3((unsigned)((n_op + GL_NODE_BLOCK / WAVE - 1) / (GL_NODE_BLOCK / WAVE))), dim3(GL_NODE_BLOCK), 0, st, d_st, d_par, n_op, WC, d_node);
		PANCHK(m, hipGetLastError());
		if (g0 == 0 && in->st_rows != nullptr) { // tests only: the first chunk's state rows
			PANCHK(m, hipMemcpyAsync(in->st_rows, d_st, sizeof(uint64_t) * n_row, hipMemcpyDeviceToHost, st));
			PANCHK(m, hipStreamSynchronize(st));
		}
	}
	PANCHK(m, hipMemcpyAsync(h_gene, d_gene, sizeof(int32_t) * n_gene4, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipMemcpyAsync(h_node, d_node, sizeof(int64_t) * n_node3, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	return 0;
}
