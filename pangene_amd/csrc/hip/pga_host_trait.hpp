// pga_pan_trait (include/pangene_hip.h): the permutation test of pangene trait on the device (k_trait.hpp).  Context-free: it runs on a
// stream of its own on the current device.  The device buffers and the page-locked results are kept from call to call and only ever
// grow; pga_host_trim(0) gives them back.  The results wait in the page-locked buffers until the next call.
//
// The permutations go through in batches of pga_trait_batch() label rows (65 536, or PANGENE_TRAIT_BATCH=n up to 4 194 304), so device memory is
// bounded by G, N and the batch and not by n: per batch k_trait_perm makes the rows and k_trait_count counts them against every gene,
// one after the other on the one stream.  Nothing is read back between the batches; a, s and k come down once at the end.

constexpr int32_t TRAIT_MAX_COL = 16777215, TRAIT_MAX_GENE = 16777215;
constexpr int32_t TRAIT_BATCH = 65536;

struct TraitBuf { enum { BITS, LABEL, A, S, LO, HI, K, ROWS, WORK, N_BUF }; }; // page-locked buffer 0: a, s, k

extern "C" int32_t pga_trait_batch(void) { return (int32_t)pan_env("PANGENE_TRAIT_BATCH", TRAIT_BATCH, 1 << 22); }

extern "C" int pga_pan_trait(const pga_trait_in_t *in, pga_trait_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->a = out->s = out->k = nullptr;
	if (in == nullptr) return PGA_ERR_ARG;
	const int32_t G = in->n_gene, N = in->n_col, n = in->n_perm;
	if (G < 0 || N < 0 || n < 0 || in->min_count < 1) return PGA_ERR_ARG;
	if (N > TRAIT_MAX_COL || G > TRAIT_MAX_GENE || n > PAN_MAX_PERM) return PGA_ERR_RANGE;
	const int32_t W = (N + 31) / 32;
	if (W > 0 && ((G > 0 && in->bits == nullptr) || in->label == nullptr)) return PGA_ERR_ARG;
	PanDev &m = g_pan[PAN_TRAIT];
	std::lock_guard<std::mutex> lk(m.mu);
	int32_t *h_res = m.get_host<int32_t>(0, (size_t)G * 3);
	PANMEM(h_res);
	out->a = h_res, out->s = h_res + G, out->k = h_res + 2 * (size_t)G;
	memset(h_res, 0, sizeof(int32_t) * 3 * (size_t)G);
	if (G == 0 && in->perm_rows == nullptr) return 0;
	if (W == 0) return 0; // no columns: every count is 0
	int32_t t_sum = 0;
	for (int32_t k = 0; k < W; ++k) t_sum += __builtin_popcount(in->label[k]);
	hipStream_t st;
	PANCHK(m, m.stream(&st));

	const size_t n_word = (size_t)G * (size_t)W;
	PermBatches b(n, pga_trait_batch(), W <= TRAIT_PERM_LDS_W);
	uint32_t *d_bits = m.get<uint32_t>(TraitBuf::BITS, n_word), *d_label = m.get<uint32_t>(TraitBuf::LABEL, (size_t)W);
	int32_t *d_a = m.get<int32_t>(TraitBuf::A, (size_t)G), *d_s = m.get<int32_t>(TraitBuf::S, (size_t)G), *d_lo = m.get<int32_t>(TraitBuf::LO, (size_t)G);
	int32_t *d_hi = m.get<int32_t>(TraitBuf::HI, (size_t)G), *d_k = m.get<int32_t>(TraitBuf::K, (size_t)G);
	uint32_t *d_rows = m.get<uint32_t>(TraitBuf::ROWS, (size_t)b.B * (size_t)W);
	uint32_t *d_work = m.get<uint32_t>(TraitBuf::WORK, b.work((size_t)W));
	PANMEM(d_bits); PANMEM(d_label); PANMEM(d_a); PANMEM(d_s); PANMEM(d_lo); PANMEM(d_hi); PANMEM(d_k); PANMEM(d_rows); PANMEM(d_work);
	if (n_word) PANCHK(m, hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * n_word, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_label, in->label, sizeof(uint32_t) * (size_t)W, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_k, 0, sizeof(int32_t) * (size_t)(G ? G : 1), st));
	if (G > 0) {
		const unsigned row_blocks = (unsigned)(((int64_t)G + BLOCK / TRAIT_ROW_LANES - 1) / (BLOCK / TRAIT_ROW_LANES));
		hipLaunchKernelGGL(k_trait_obs, dim3(row_blocks), dim3(BLOCK), 0, st, d_bits, d_label, G, W, N, t_sum, in->min_count, d_a, d_s, d_lo, d_hi);
	}
	const int32_t n_chunk = (W + DIST_KC - 1) / DIST_KC;
	const unsigned gene_tiles = (unsigned)((G + DIST_TILE - 1) / DIST_TILE);
	for (; b.more(); b.next()) {
		const int32_t nb = b.nb();
		perm_launch(b.lds, k_trait_perm<true>, k_trait_perm<false>, nb, st, d_label, N, W, in->seed, b.p0(), nb, d_work, d_rows);
		if (b.first() && in->perm_rows != nullptr) { // tests only: the label rows of the first batch
			PANCHK(m, hipGetLastError());
			PANCHK(m, hipMemcpyAsync(in->perm_rows, d_rows, sizeof(uint32_t) * (size_t)nb * (size_t)W, hipMemcpyDeviceToHost, st));
			PANCHK(m, hipStreamSynchronize(st));
		}
		if (G > 0)
			hipLaunchKernelGGL(k_trait_count, dim3(gene_tiles, (unsigned)((nb + DIST_TILE - 1) / DIST_TILE)), dim3(BLOCK), 0, st, d_bits, d_rows, d_lo, d_hi, G, nb, W,
			                   n_chunk, d_k);
		PANCHK(m, hipGetLastError());
	}
	return pan_download3(m, st, h_res, d_a, d_s, d_k, G);
}
