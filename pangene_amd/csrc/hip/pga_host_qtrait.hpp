// pga_pan_qtrait (include/pangene_hip.h): the rank-sum permutation test of pangene qtrait on the device (k_qtrait.hpp).  Context-free: it
// runs on a stream of its own on the current device.  The device buffers and the page-locked results are kept from call to call and only
// ever grow; pga_host_trim(0) gives them back.  The results wait in the page-locked buffer until the next call.
//
// The permutations go through in batches of pga_qtrait_batch() rows (16 384, or PANGENE_QTRAIT_BATCH=n up to 1 048 576): per batch
// k_qtrait_perm makes the digit planes and k_qtrait_count multiplies them with every gene row, one after the other on the one stream.
// Nothing is read back between the batches and the host waits once, at the end (tests that ask for perm_rows / d_rows wait once more, in
// the first batch).  The default: a batch is 128 permutation tiles, which with the 40 gene tiles of 5 000 genes is 5 120 workgroups,
// ten rounds of the 512 a chip holds at two per CU, and its two planes take 2 x 16 384 x K bytes -- 1 GiB at the limit of
// K = 32 000 where trait's 65 536 rows would take 4 GiB.
constexpr int32_t QTRAIT_MAX_COL = 32000, QTRAIT_MAX_GENE = 16777215;
constexpr int32_t QTRAIT_BATCH = 16384;

struct QtraitBuf { enum { BITS, C2, A, D, ABSD, K, LO, HI, WORK, DROWS, N_BUF }; }; // page-locked buffer 0: a, d, k; 1: the planes (tests)

extern "C" int32_t pga_qtrait_batch(void) { return (int32_t)pan_env("PANGENE_QTRAIT_BATCH", QTRAIT_BATCH, 1 << 20); }

extern "C" int pga_pan_qtrait(const pga_qtrait_in_t *in, pga_qtrait_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->a = out->d = out->k = nullptr;
	if (in == nullptr) return PGA_ERR_ARG;
	const int32_t G = in->n_gene, N = in->n_col, n = in->n_perm;
	if (G < 0 || N < 0 || n < 0 || in->min_count < 1) return PGA_ERR_ARG;
	if (N > QTRAIT_MAX_COL || G > QTRAIT_MAX_GENE || n > PAN_MAX_PERM) return PGA_ERR_RANGE; // (before anything is launched)
	const int32_t W = (N + 31) / 32;
	if (W > 0 && ((G > 0 && in->bits == nullptr) || in->c2 == nullptr)) return PGA_ERR_ARG;
	PanDev &m = g_pan[PAN_QTRAIT];
	std::lock_guard<std::mutex> lk(m.mu);
	int32_t *h_res = m.get_host<int32_t>(0, (size_t)G * 3);
	PANMEM(h_res);
	out->a = h_res, out->d = h_res + G, out->k = h_res + 2 * (size_t)G;
	memset(h_res, 0, sizeof(int32_t) * 3 * (size_t)G);
	if (G == 0 && in->perm_rows == nullptr) return 0;
	if (W == 0) return 0; // no columns: every sum is 0
	hipStream_t st;
	PANCHK(m, m.stream(&st));

	// K: the columns of a plane row, N rounded up to the count kernel's K chunk.  k_qtrait_perm writes zeros past N; what stands there
	// would not matter, because the gene side is zero there: bits past N are zero in the rows and words past W are staged as zero.
	const int32_t K = (N + QT_KC - 1) / QT_KC * QT_KC;
	const size_t n_word = (size_t)G * (size_t)W;
	PermBatches b(n, pga_qtrait_batch(), N <= QT_PERM_LDS_N);
	const bool tests_d = in->d_rows != nullptr && G > 0;
	uint32_t *d_bits = m.get<uint32_t>(QtraitBuf::BITS, n_word);
	int16_t *d_c2 = m.get<int16_t>(QtraitBuf::C2, (size_t)W * 32); // (k_qtrait_obs indexes it by bit position: whole words, zero past N)
	int32_t *d_a = m.get<int32_t>(QtraitBuf::A, (size_t)G), *d_d = m.get<int32_t>(QtraitBuf::D, (size_t)G), *d_abs = m.get<int32_t>(QtraitBuf::ABSD, (size_t)G);
	int32_t *d_k = m.get<int32_t>(QtraitBuf::K, (size_t)G);
	int8_t *d_lo = m.get<int8_t>(QtraitBuf::LO, (size_t)b.B * (size_t)K), *d_hi = m.get<int8_t>(QtraitBuf::HI, (size_t)b.B * (size_t)K);
	int16_t *d_work = m.get<int16_t>(QtraitBuf::WORK, b.work((size_t)N));
	int32_t *d_drows = m.get<int32_t>(QtraitBuf::DROWS, tests_d ? (size_t)b.B * (size_t)G : 1);
	PANMEM(d_bits); PANMEM(d_c2); PANMEM(d_a); PANMEM(d_d); PANMEM(d_abs); PANMEM(d_k); PANMEM(d_lo); PANMEM(d_hi); PANMEM(d_work); PANMEM(d_drows);
	if (n_word) PANCHK(m, hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * n_word, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_c2, 0, sizeof(int16_t) * (size_t)W * 32, st));
	PANCHK(m, hipMemcpyAsync(d_c2, in->c2, sizeof(int16_t) * (size_t)N, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_k, 0, sizeof(int32_t) * (size_t)(G ? G : 1), st));
	if (G > 0) {
		const unsigned row_blocks = (unsigned)(((int64_t)G + BLOCK / QT_ROW_LANES - 1) / (BLOCK / QT_ROW_LANES));
		hipLaunchKernelGGL(k_qtrait_obs, dim3(row_blocks), dim3(BLOCK), 0, st, d_bits, d_c2, G, W, N, in->min_count, d_a, d_d, d_abs);
	}
	const unsigned gene_tiles = (unsigned)((G + QT_TILE - 1) / QT_TILE);
	const bool use_hi = N >= QT_HI_FROM;
	for (; b.more(); b.next()) {
		const int32_t nb = b.nb();
		const bool first = b.first();
		perm_launch(b.lds, k_qtrait_perm<true>, k_qtrait_perm<false>, nb, st, d_c2, N, K, in->seed, b.p0(), nb, d_work, d_lo, d_hi);
		int32_t *dr = first && tests_d ? d_drows : nullptr;
		if (G > 0) {
			const dim3 grid(gene_tiles, (unsigned)((nb + QT_TILE - 1) / QT_TILE));
			if (use_hi) hipLaunchKernelGGL(k_qtrait_count<true>, grid, dim3(BLOCK), 0, st, d_bits, d_lo, d_hi, d_abs, G, nb, W, K, d_k, dr);
			else hipLaunchKernelGGL(k_qtrait_count<false>, grid, dim3(BLOCK), 0, st, d_bits, d_lo, d_hi, d_abs, G, nb, W, K, d_k, dr);
		}
		PANCHK(m, hipGetLastError());
		if (first && (in->perm_rows != nullptr || dr != nullptr)) { // tests only: the first batch's rows, put together from the planes, and its D_p
			const size_t plane = (size_t)nb * (size_t)K;
			int8_t *h_pl = m.get_host<int8_t>(1, 2 * plane);
			PANMEM(h_pl);
			PANCHK(m, hipMemcpyAsync(h_pl, d_lo, plane, hipMemcpyDeviceToHost, st));
			PANCHK(m, hipMemcpyAsync(h_pl + plane, d_hi, plane, hipMemcpyDeviceToHost, st));
			if (dr) PANCHK(m, hipMemcpyAsync(in->d_rows, dr, sizeof(int32_t) * (size_t)nb * (size_t)G, hipMemcpyDeviceToHost, st));
			PANCHK(m, hipStreamSynchronize(st));
			if (in->perm_rows != nullptr)
				for (int32_t q = 0; q < nb; ++q)
					for (int32_t c = 0; c < N; ++c)
						in->perm_rows[(size_t)q * (size_t)N + (size_t)c] = (int16_t)(256 * (int32_t)h_pl[plane + (size_t)q * K + c] + (int32_t)h_pl[(size_t)q * K + c]);
		}
	}
	return pan_download3(m, st, h_res, d_a, d_d, d_k, G);
}
