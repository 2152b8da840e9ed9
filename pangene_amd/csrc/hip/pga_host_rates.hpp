// pga_pan_rates (include/pangene_hip.h): the likelihoods of a batch of parameter sets and the posteriors of set 0 on the device
// (k_rates.hpp).  Context-free: it runs on a stream of its own on the current device.  The device buffers and the page-locked staging
// and result memory are kept from call to call in the PAN_RATES pool and only ever grow; pga_host_trim(0) gives them back.  The results
// wait in the page-locked buffers until the next call.
//
// The host checks the program as pan_gainloss does, finds the depth it needs and, on the walk that checks par, the sibling of every op;
// it checks the tables and uploads everything.  Without post ONE launch of k_rt_up covers all items and sets.  With post the items go
// through in chunks, so that rows -- 16 bytes per item and node -- stays bounded: per chunk k_rt_up, k_rt_down and k_rt_node follow each
// other on the one stream, and k_rt_node adds the chunk's node totals into node.  Nothing is read back between the chunks and the host
// waits once, at the end (tests that ask for post_rows wait once more, after the first chunk).
constexpr int64_t RT_ROW_BYTES = (int64_t)1 << 30; // what rows of one chunk may take

struct RatesBuf {
	enum { OPS, SIB, BITS, TAB, PI, ROWS, PART, LIKM, LIKE, GENE, NODE, PRES, N_BUF };
	enum { H_IN, H_LIK, H_POST }; // page-locked: the packed program and the siblings; lik_m and lik_e; gene and node
};
static_assert(RatesBuf::N_BUF <= PAN_MAX_DEV, "the pool has no room for the rates buffers");

// items per chunk of a call with post over a tree of n_leaf leaves: PANGENE_RATES_CHUNK (rounded up to a multiple of 256), or the
// largest multiple of 256 whose 16 (2 n_leaf - 1) bytes per item fit RT_ROW_BYTES; never less than 256
extern "C" int32_t pga_rates_chunk(int32_t n_leaf)
{
	const int64_t n_op = std::max<int64_t>(2 * (int64_t)n_leaf - 1, 1);
	const int64_t fit = std::min<int64_t>(RT_ROW_BYTES / (16 * n_op), (int64_t)1 << 24) / 256 * 256;
	const int64_t c = pan_env("PANGENE_RATES_CHUNK", std::max<int64_t>(fit, 256), (int64_t)1 << 24);
	return (int32_t)((c + 255) / 256 * 256);
}

extern "C" int pga_pan_rates(const pga_rates_in_t *in, pga_rates_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->lik_m = nullptr, out->lik_e = nullptr, out->gene = nullptr, out->node = nullptr;
	if (in == nullptr) return PGA_ERR_ARG;
	const int32_t G = in->n_gene, L = in->n_leaf, S = in->n_set;
	if (G < 0 || L < 0 || S < 1) return PGA_ERR_ARG;
	if (L > GL_MAX_LEAF || G > GL_MAX_GENE || S > RT_MAX_SET) return PGA_ERR_RANGE;
	if ((in->post != 0 && in->post != 1) || in->n_sum < 0 || in->n_sum > G) return PGA_ERR_ARG;
	const int32_t W = (G + 31) / 32, n_op = L > 0 ? 2 * L - 1 : 0, OW = (n_op + 31) / 32;
	if (L > 0 && (in->op == nullptr || in->par == nullptr || in->tab == nullptr || in->pi == nullptr || (G > 0 && in->bits == nullptr))) return PGA_ERR_ARG;
	// the program: n_leaf pushes, no join of fewer than two entries, one entry left; the depth it needs; par names the join that takes a
	// node, and the two nodes a join takes are each other's siblings
	int32_t depth = 0, pushed = 0;
	std::vector<int32_t> made, sib((size_t)n_op, -1);
	for (int32_t k = 0; k < n_op; ++k) {
		if (in->op[k] == 0) ++pushed, made.push_back(k), depth = std::max(depth, (int32_t)made.size());
		else if (in->op[k] == 1 && made.size() >= 2) {
			const int32_t a = made[made.size() - 2], b = made.back();
			if (in->par[a] != k || in->par[b] != k) return PGA_ERR_ARG;
			sib[(size_t)a] = b, sib[(size_t)b] = a;
			made.pop_back(), made.back() = k;
		} else return PGA_ERR_ARG;
	}
	if (n_op > 0 && (made.size() != 1 || pushed != L || in->par[n_op - 1] != -1)) return PGA_ERR_ARG;
	if (depth > RT_DEPTH) return PGA_ERR_RANGE;
	const size_t n_tab = (size_t)S * (size_t)n_op * 4;
	for (size_t i = 0; i < n_tab; ++i)
		if (!(std::isfinite(in->tab[i]) && in->tab[i] >= 0.0)) return PGA_ERR_ARG;
	for (size_t i = 0; n_op > 0 && i < 2 * (size_t)S; ++i)
		if (!(std::isfinite(in->pi[i]) && in->pi[i] >= 0.0)) return PGA_ERR_ARG;
	PanDev &m = g_pan[PAN_RATES];
	std::lock_guard<std::mutex> lk(m.mu);
	const size_t n_lik = (size_t)S * (size_t)G, n_gene3 = (size_t)G * 3, n_node3 = (size_t)n_op * 3;
	// lik_e behind lik_m, node behind gene
	double *h_lik = m.get_host<double>(RatesBuf::H_LIK, n_lik + (n_lik + 1) / 2);
	double *h_post = m.get_host<double>(RatesBuf::H_POST, n_gene3 + n_node3);
	PANMEM(h_lik); PANMEM(h_post);
	int32_t *h_like = (int32_t *)(h_lik + n_lik);
	out->lik_m = h_lik, out->lik_e = h_like;
	if (in->post) out->gene = h_post, out->node = h_post + n_gene3;
	memset(h_lik, 0, sizeof(double) * n_lik);
	memset(h_like, 0, sizeof(int32_t) * n_lik);
	memset(h_post, 0, sizeof(double) * (n_gene3 + n_node3));
	if (G == 0 || L == 0) return 0; // nothing to do: no launch
	uint32_t *h_in = m.get_host<uint32_t>(RatesBuf::H_IN, (size_t)OW + (size_t)n_op);
	PANMEM(h_in);
	memset(h_in, 0, sizeof(uint32_t) * (size_t)OW);
	for (int32_t k = 0; k < n_op; ++k) h_in[k >> 5] |= (uint32_t)in->op[k] << (k & 31);
	memcpy(h_in + OW, sib.data(), sizeof(int32_t) * (size_t)n_op);
	const int32_t chunk = in->post ? pga_rates_chunk(L) : G;
	const int32_t G1 = std::min(chunk, G); // the largest chunk
	const int32_t WW = (G1 + WAVE - 1) / WAVE;
	const size_t n_row = in->post ? (size_t)n_op * (size_t)G1 : 0, n_part = in->post ? (size_t)n_op * (size_t)WW * 3 : 0, n_word = (size_t)L * (size_t)W;
	const bool want_pres = in->post && in->post_rows != nullptr;
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	uint32_t *d_ops = m.get<uint32_t>(RatesBuf::OPS, (size_t)OW), *d_bits = m.get<uint32_t>(RatesBuf::BITS, n_word);
	int32_t *d_sib = m.get<int32_t>(RatesBuf::SIB, (size_t)n_op), *d_like = m.get<int32_t>(RatesBuf::LIKE, n_lik);
	double *d_tab = m.get<double>(RatesBuf::TAB, n_tab), *d_pi = m.get<double>(RatesBuf::PI, 2 * (size_t)S), *d_likm = m.get<double>(RatesBuf::LIKM, n_lik);
	double2 *d_rows = m.get<double2>(RatesBuf::ROWS, n_row);
	double *d_part = m.get<double>(RatesBuf::PART, n_part), *d_gene = m.get<double>(RatesBuf::GENE, in->post ? n_gene3 : 0);
	double *d_node = m.get<double>(RatesBuf::NODE, in->post ? n_node3 : 0), *d_pres = m.get<double>(RatesBuf::PRES, want_pres ? n_row : 0);
	PANMEM(d_ops); PANMEM(d_bits); PANMEM(d_sib); PANMEM(d_like); PANMEM(d_tab); PANMEM(d_pi); PANMEM(d_likm); PANMEM(d_rows); PANMEM(d_part); PANMEM(d_gene);
	PANMEM(d_node); PANMEM(d_pres);
	PANCHK(m, hipMemcpyAsync(d_ops, h_in, sizeof(uint32_t) * (size_t)OW, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_sib, h_in + OW, sizeof(int32_t) * (size_t)n_op, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * n_word, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_tab, in->tab, sizeof(double) * n_tab, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_pi, in->pi, sizeof(double) * 2 * (size_t)S, hipMemcpyHostToDevice, st));
	if (in->post) PANCHK(m, hipMemsetAsync(d_node, 0, sizeof(double) * n_node3, st));
	const int32_t n_slot = std::max(depth - 1, 1);
	const size_t lds_up = (sizeof(double) * 2 + sizeof(int32_t)) * RT_BLOCK * (size_t)n_slot, lds_down = sizeof(double) * 2 * RT_BLOCK * (size_t)n_slot;
	// PANGENE_RATES_TIMING: events around the three kernels of every chunk, read after the call's one wait
	const bool timing = getenv("PANGENE_RATES_TIMING") != nullptr;
	std::vector<hipEvent_t> ev;
	auto mark = [&]() {
		if (!timing) return hipSuccess;
		hipEvent_t e;
		hipError_t rc = hipEventCreate(&e);
		if (rc == hipSuccess) ev.push_back(e), rc = hipEventRecord(e, st);
		return rc;
	};
	for (int32_t g0 = 0; g0 < G; g0 += chunk) {
		const int32_t Gc = std::min(chunk, G - g0);
		const int32_t WC = (Gc + WAVE - 1) / WAVE; // the chunk's rows are Gc items long, its partials WC waves
		const unsigned blocks = (unsigned)((Gc + RT_BLOCK - 1) / RT_BLOCK);
		PANCHK(m, mark());
		hipLaunchKernelGGL(k_rt_up, dim3(blocks, (unsigned)S), dim3(RT_BLOCK), lds_up, st, d_ops, d_bits, g0, Gc, G, W, L, n_op, n_slot, d_tab, d_pi, d_likm, d_like,
		                   in->post ? d_rows : (double2 *)nullptr);
		PANCHK(m, mark());
		if (in->post) {
			hipLaunchKernelGGL(k_rt_down, dim3(blocks), dim3(RT_BLOCK), lds_down, st, d_ops, d_sib, g0, Gc, n_op, in->n_sum, WC, d_tab, d_pi, d_rows, d_part, d_gene,
			                   want_pres && g0 == 0 ? d_pres : (double *)nullptr);
			PANCHK(m, mark());
			hipLaunchKernelGGL(k_rt_node, dim3((unsigned)((n_op + RT_NODE_BLOCK / WAVE - 1) / (RT_NODE_BLOCK / WAVE))), dim3(RT_NODE_BLOCK), 0, st, d_part, n_op, WC, d_node);
			PANCHK(m, mark());
		}
		PANCHK(m, hipGetLastError());
		if (g0 == 0 && want_pres) { // tests only: the first chunk's posterior presence
			PANCHK(m, hipMemcpyAsync(in->post_rows, d_pres, sizeof(double) * (size_t)n_op * (size_t)Gc, hipMemcpyDeviceToHost, st));
			PANCHK(m, hipStreamSynchronize(st));
		}
	}
	PANCHK(m, hipMemcpyAsync(h_lik, d_likm, sizeof(double) * n_lik, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipMemcpyAsync(h_like, d_like, sizeof(int32_t) * n_lik, hipMemcpyDeviceToHost, st));
	if (in->post) {
		PANCHK(m, hipMemcpyAsync(h_post, d_gene, sizeof(double) * n_gene3, hipMemcpyDeviceToHost, st));
		PANCHK(m, hipMemcpyAsync(h_post + n_gene3, d_node, sizeof(double) * n_node3, hipMemcpyDeviceToHost, st));
	}
	PANCHK(m, hipStreamSynchronize(st));
	if (timing) {
		double t[3] = {0, 0, 0};
		const size_t per = in->post ? 4 : 2;
		for (size_t i = 0; i + 1 < ev.size(); ++i) {
			if (i % per == per - 1) continue; // (between two chunks)
			float ms = 0;
			if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess) t[i % per] += ms;
		}
		for (hipEvent_t e : ev) (void)hipEventDestroy(e);
		fprintf(stderr, "[rates-kernels] items=%d leaves=%d sets=%d post=%d chunk=%d up_ms=%.3f down_ms=%.3f node_ms=%.3f\n", G, L, S, in->post, chunk, t[0], t[1], t[2]);
	}
	return 0;
}
