// pga_pan_glm (include/pangene_hip.h): the score statistics of pangene glm on the device (k_glm.hpp).  Context-free: it runs on a stream
// of its own on the current device.  The device buffers and the page-locked results are kept from call to call and only ever grow;
// pga_host_trim(0) gives them back.  The results wait in the page-locked buffer until the next call.
//
// One call is two launches and one wait: k_glm_sums over (gene blocks, traits, K segments), k_glm_stat over (gene blocks, traits).  The
// split over the assemblies depends on the shape alone -- segments of whole chunks, as many as bring the grid to two workgroups per CU
// on 256 CUs -- so the same call returns the same bits.
constexpr int32_t GLM_MAX_COL = 16384, GLM_MAX_GENE = 16777215, GLM_MAX_TRAIT = 4096;

struct GlmBuf { enum { BITS, COLS, CHOL, PART, A, U, V, SW, SUMS, N_BUF }; }; // page-locked buffer 0: u, v, sw, a

extern "C" int pga_pan_glm(const pga_glm_in_t *in, pga_glm_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->a = nullptr, out->u = out->v = out->sw = nullptr;
	if (in == nullptr) return PGA_ERR_ARG;
	const int32_t G = in->n_gene, A = in->n_asm, T = in->n_trait, k = in->n_cov;
	if (G < 0 || A < 0 || T < 0 || k < 0) return PGA_ERR_ARG;
	if (A > GLM_MAX_COL || k > GLM_MAX_COV || G > GLM_MAX_GENE || T > GLM_MAX_TRAIT) return PGA_ERR_RANGE; // (before anything is launched)
	const int32_t W = (A + 31) / 32, k1 = k + 1;
	const size_t tg = (size_t)T * (size_t)G;
	if (tg > 0 && A > 0 && (in->bits == nullptr || in->cols == nullptr)) return PGA_ERR_ARG;
	if (tg > 0 && in->chol == nullptr) return PGA_ERR_ARG;
	PanDev &m = g_pan[PAN_GLM];
	std::lock_guard<std::mutex> lk(m.mu);
	double *h_res = m.get_host<double>(0, 3 * tg + (tg + 1) / 2);
	PANMEM(h_res);
	out->u = h_res, out->v = h_res + tg, out->sw = h_res + 2 * tg, out->a = (const int32_t *)(h_res + 3 * tg);
	memset(h_res, 0, sizeof(double) * (3 * tg + (tg + 1) / 2));
	if (tg == 0) return 0;
	if (A == 0) { // no assemblies: every sum is 0
		if (in->sums_test != nullptr) memset(in->sums_test, 0, sizeof(double) * tg * GLM_COLS);
		return 0;
	}
	hipStream_t st;
	PANCHK(m, m.stream(&st));

	const int32_t n_chunk = (A + GLM_KC - 1) / GLM_KC, a_pad = n_chunk * GLM_KC;
	const int64_t blocks = (int64_t)((G + GLM_GENES - 1) / GLM_GENES) * T, want = 512;
	int32_t n_seg = blocks >= want ? 1 : (int32_t)std::min<int64_t>(n_chunk, (want + blocks - 1) / blocks);
	const int32_t cps = (n_chunk + n_seg - 1) / n_seg;
	n_seg = (n_chunk + cps - 1) / cps; // no empty segment
	const size_t n_word = (size_t)G * (size_t)W, n_col = (size_t)T * (size_t)a_pad * GLM_COLS, n_chol = (size_t)T * (size_t)(k1 * k1);
	uint32_t *d_bits = m.get<uint32_t>(GlmBuf::BITS, n_word);
	double *d_cols = m.get<double>(GlmBuf::COLS, n_col), *d_chol = m.get<double>(GlmBuf::CHOL, n_chol);
	double *d_part = m.get<double>(GlmBuf::PART, (size_t)n_seg * tg * GLM_COLS);
	int32_t *d_a = m.get<int32_t>(GlmBuf::A, tg);
	double *d_u = m.get<double>(GlmBuf::U, tg), *d_v = m.get<double>(GlmBuf::V, tg), *d_sw = m.get<double>(GlmBuf::SW, tg);
	double *d_sums = m.get<double>(GlmBuf::SUMS, in->sums_test != nullptr ? tg * GLM_COLS : 1);
	PANMEM(d_bits); PANMEM(d_cols); PANMEM(d_chol); PANMEM(d_part); PANMEM(d_a); PANMEM(d_u); PANMEM(d_v); PANMEM(d_sw); PANMEM(d_sums);
	PANCHK(m, hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * n_word, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_cols, 0, sizeof(double) * n_col, st)); // (the rows past the assemblies must be zero: 0 x anything else is not)
	const size_t row_in = sizeof(double) * (size_t)A * GLM_COLS, row_dev = sizeof(double) * (size_t)a_pad * GLM_COLS;
	PANCHK(m, hipMemcpy2DAsync(d_cols, row_dev, in->cols, row_in, row_in, (size_t)T, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_chol, in->chol, sizeof(double) * n_chol, hipMemcpyHostToDevice, st));
	const unsigned gene_blocks = (unsigned)((G + GLM_GENES - 1) / GLM_GENES);
	const bool timing = getenv("PANGENE_GLM_TIMING") != nullptr; // one [glm-kernels] line on stderr: the device time of the two kernels
	hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
	if (timing) for (hipEvent_t &e : ev) PANCHK(m, hipEventCreate(&e));
	if (timing) PANCHK(m, hipEventRecord(ev[0], st));
	hipLaunchKernelGGL(k_glm_sums, dim3(gene_blocks, (unsigned)T, (unsigned)n_seg), dim3(BLOCK), 0, st, d_bits, d_cols, G, W, a_pad, cps, d_part);
	if (timing) PANCHK(m, hipEventRecord(ev[1], st));
	hipLaunchKernelGGL(k_glm_stat, dim3((unsigned)((G + BLOCK - 1) / BLOCK), (unsigned)T), dim3(BLOCK), 0, st, d_part, d_chol, G, n_seg, k1, d_a, d_u, d_v, d_sw,
	                   in->sums_test != nullptr ? d_sums : nullptr);
	if (timing) PANCHK(m, hipEventRecord(ev[2], st));
	PANCHK(m, hipGetLastError());
	PANCHK(m, hipMemcpyAsync(h_res, d_u, sizeof(double) * tg, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipMemcpyAsync(h_res + tg, d_v, sizeof(double) * tg, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipMemcpyAsync(h_res + 2 * tg, d_sw, sizeof(double) * tg, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipMemcpyAsync(h_res + 3 * tg, d_a, sizeof(int32_t) * tg, hipMemcpyDeviceToHost, st));
	if (in->sums_test != nullptr) PANCHK(m, hipMemcpyAsync(in->sums_test, d_sums, sizeof(double) * tg * GLM_COLS, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	if (timing) {
		float sums_ms = 0, stat_ms = 0;
		PANCHK(m, hipEventElapsedTime(&sums_ms, ev[0], ev[1]));
		PANCHK(m, hipEventElapsedTime(&stat_ms, ev[1], ev[2]));
		for (hipEvent_t e : ev) (void)hipEventDestroy(e);
		fprintf(stderr, "[glm-kernels] genes=%d assemblies=%d traits=%d cov=%d gene_blocks=%u segments=%d chunks_per_segment=%d sums_ms=%.4f stat_ms=%.4f\n", G, A, T, k, gene_blocks,
		        n_seg, cps, sums_ms, stat_ms);
	}
	return 0;
}
