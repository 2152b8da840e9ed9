// pga_pan_boot (include/pangene_hip.h): the bootstrap replicates of pangene tree on the device (k_boot.hpp and the batched twins of
// k_join.hpp).  Context-free: it runs on a stream of its own on the current device.  The device buffers and the page-locked records are
// kept from call to call and only ever grow; pga_host_trim(0) gives them back.  The records wait in the page-locked buffer until the
// next call.
//
// One call takes up to pga_boot_batch(n_asm) replicates.  Draws, resampled rows, counts and distances are made replicate group by
// replicate group (a group's draws and rows stay within BOOT_ROWS_WORDS, or PANGENE_BOOT_ROWS_WORDS: tests reach a second group at a
// small input), then the joins of ALL replicates of the call are queued together: they share the live count r at every step, so the host sizes every grid without reading anything back, and waits once.

constexpr int32_t BOOT_MAX_BATCH = 1024;              // replicates a call takes at the most (the y extent of the batched grids)
constexpr int64_t BOOT_BUDGET = (int64_t)2 << 30;     // device memory of a call's replicates: what pga_boot_batch divides
constexpr int64_t BOOT_ROWS_WORDS = (int64_t)64 << 20; // draws + resampled rows of a replicate group: 256 MiB, or one replicate's

// REC: the records, then one flag word per replicate; page-locked buffer 0: the same
struct BootBuf { enum { BITS, DRAWS, ROWS, S, D, LABEL, AUX, PART, REC, MX, N_BUF }; };

// Replicates per call: the budget over what a replicate keeps for the whole call -- S (A^2 words), d (A x ld), label, aux, the search's
// candidates and the records.  The draws and the resampled rows are not in it: the function takes n_asm alone and their size depends on
// n_item, so they are bounded apart (BOOT_ROWS_WORDS).  A call's device memory is therefore at most the 2 GiB of the budget, the
// A x W words of the bit rows, and 256 MiB of draws and rows -- or one replicate's draws and rows (n_item + A x W words) if that is more.
extern "C" int32_t pga_boot_batch(int32_t n_asm)
{
	const int64_t A = std::max(n_asm, 1), ld = (A + 3) & ~(int64_t)3;
	const int64_t per = 4 * A * A + 4 * A * ld + 12 * A + (int64_t)sizeof(JoinPart) * JOIN_MAX_PART + 48 * A + 8;
	return (int32_t)pan_env("PANGENE_BOOT_BATCH", std::min<int64_t>(std::max<int64_t>(BOOT_BUDGET / per, 1), BOOT_MAX_BATCH), BOOT_MAX_BATCH);
}

// words of the source row's LDS window: BOOT_LDS_WORDS, or PANGENE_BOOT_LDS_WORDS (tests: the global path at a small n_item)
static int32_t boot_lds_words() { return (int32_t)pan_env("PANGENE_BOOT_LDS_WORDS", BOOT_LDS_WORDS, BOOT_LDS_WORDS); }

// words of draws + resampled rows a replicate group may take: BOOT_ROWS_WORDS, or PANGENE_BOOT_ROWS_WORDS (tests: several groups in a call)
static int64_t boot_rows_words() { return pan_env("PANGENE_BOOT_ROWS_WORDS", BOOT_ROWS_WORDS, BOOT_ROWS_WORDS); }

template <bool NJ>
static int boot_join_queue(hipStream_t st, int32_t *d_d, int32_t n, int32_t ld, int32_t n_rep, int32_t *d_label, long long *d_aux, JoinPart *d_part, int32_t p_stride,
                           long long *d_rec, size_t rec_stride, int32_t *d_flag)
{
	const size_t d_stride = (size_t)n * (size_t)ld;
	const unsigned B = (unsigned)n_rep;
	hipLaunchKernelGGL(k_join_init_b<NJ>, dim3((unsigned)n, B), dim3(BLOCK), 0, st, d_d, n, ld, d_label, d_aux, d_flag, d_stride, n);
	PANCHK(g_pan[PAN_BOOT], hipGetLastError());
	int32_t s = 0;
	for (int32_t r = n; r > (NJ ? 3 : 1); --r, ++s) {
		const int32_t n_tile = ((r + JOIN_CW - 1) / JOIN_CW) * ((r + JOIN_RB - 1) / JOIN_RB), n_part = std::min(n_tile, p_stride);
		hipLaunchKernelGGL(k_join_argmin_b<NJ>, dim3((unsigned)n_part, B), dim3(BLOCK), 0, st, d_d, ld, r, d_label, d_aux, d_part, d_stride, n, p_stride);
		hipLaunchKernelGGL(k_join_update_b<NJ>, dim3((unsigned)((r + BLOCK - 1) / BLOCK), B), dim3(BLOCK), 0, st, d_d, ld, r, d_label, d_aux, d_part, n_part,
		                   d_rec + 6 * (size_t)s, d_flag, d_stride, n, p_stride, rec_stride);
		if ((s & 255) == 255) PANCHK(g_pan[PAN_BOOT], hipGetLastError());
	}
	if (NJ) hipLaunchKernelGGL(k_join_final_b, dim3(1, B), dim3(WAVE), 0, st, d_d, ld, d_label, d_rec + 6 * (size_t)s, d_stride, n, rec_stride);
	PANCHK(g_pan[PAN_BOOT], hipGetLastError());
	return 0;
}

extern "C" int pga_pan_boot(const pga_boot_in_t *in, pga_boot_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	out->rec = nullptr, out->n_rec = 0;
	if (in == nullptr || in->n_item < 0 || in->n_asm < 3 || (in->metric != 0 && in->metric != 2) || (in->method != 0 && in->method != 1)) return PGA_ERR_ARG;
	if (in->n_rep < 0 || in->first < 1 || (int64_t)in->first + in->n_rep - 1 > INT32_MAX) return PGA_ERR_ARG;
	const int32_t M = in->n_item, A = in->n_asm, n_rep = in->n_rep;
	if (A > JOIN_MAX_N) return PGA_ERR_RANGE;
	if (n_rep > pga_boot_batch(A)) return PGA_ERR_ARG;
	const int32_t W = (int32_t)(((int64_t)M + 31) / 32);
	if (W > 0 && in->bits == nullptr) return PGA_ERR_ARG;
	const bool nj = in->method == 0, diff = in->metric == 2;
	const int32_t n_rec = nj ? A - 2 : A - 1, ld = (A + 3) & ~3;
	const size_t nn = (size_t)A * (size_t)A, rec_stride = 6 * (size_t)n_rec, n_flag64 = ((size_t)n_rep + 1) / 2;
	PanDev &m = g_pan[PAN_BOOT];
	std::lock_guard<std::mutex> lk(m.mu);
	int64_t *h_rec = m.get_host<int64_t>(0, rec_stride * (size_t)n_rep + n_flag64);
	PANMEM(h_rec);
	out->rec = h_rec, out->n_rec = n_rec;
	if (n_rep == 0) return 0;
	out->rec = nullptr, out->n_rec = 0;
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	// replicates of a group: its draws and rows within the rows budget, one replicate at least
	const int64_t rep_words = (int64_t)A * W + M;
	const int32_t g_max = (int32_t)std::max<int64_t>(1, std::min<int64_t>(n_rep, rep_words > 0 ? boot_rows_words() / rep_words : n_rep));
	const int32_t max_part = join_max_part();
	uint32_t *d_bits = m.get<uint32_t>(BootBuf::BITS, (size_t)A * (size_t)W), *d_rows = m.get<uint32_t>(BootBuf::ROWS, (size_t)g_max * (size_t)A * (size_t)W);
	int32_t *d_draws = m.get<int32_t>(BootBuf::DRAWS, (size_t)g_max * (size_t)M), *d_S = m.get<int32_t>(BootBuf::S, (size_t)n_rep * nn);
	int32_t *d_d = m.get<int32_t>(BootBuf::D, (size_t)n_rep * (size_t)A * (size_t)ld), *d_label = m.get<int32_t>(BootBuf::LABEL, (size_t)n_rep * (size_t)A);
	int32_t *d_mx = m.get<int32_t>(BootBuf::MX, (size_t)n_rep);
	long long *d_aux = m.get<long long>(BootBuf::AUX, (size_t)n_rep * (size_t)A), *d_rec = m.get<long long>(BootBuf::REC, rec_stride * (size_t)n_rep + n_flag64);
	JoinPart *d_part = m.get<JoinPart>(BootBuf::PART, (size_t)n_rep * (size_t)max_part);
	PANMEM(d_bits); PANMEM(d_rows); PANMEM(d_draws); PANMEM(d_S); PANMEM(d_d); PANMEM(d_label); PANMEM(d_mx); PANMEM(d_aux); PANMEM(d_rec); PANMEM(d_part);
	int32_t *d_flag = (int32_t *)(d_rec + rec_stride * (size_t)n_rep);
	PANCHK(m, hipMemsetAsync(d_flag, 0, sizeof(int64_t) * n_flag64, st));
	if (diff) PANCHK(m, hipMemsetAsync(d_mx, 0, sizeof(int32_t) * (size_t)n_rep, st));
	if (W > 0) PANCHK(m, hipMemcpyAsync(d_bits, in->bits, sizeof(uint32_t) * (size_t)A * (size_t)W, hipMemcpyHostToDevice, st));
	else PANCHK(m, hipMemsetAsync(d_S, 0, sizeof(int32_t) * (size_t)n_rep * nn, st)); // no items: every count is zero
	const DistShape sh = dist_shape(A, W);
	const bool use_lds = W <= boot_lds_words();
	const unsigned n_wc = (unsigned)((W + BLOCK - 1) / BLOCK);
	for (int32_t q0 = 0; q0 < n_rep; q0 += g_max) {
		const int32_t g = std::min(g_max, n_rep - q0);
		int32_t *S_g = d_S + (size_t)q0 * nn;
		if (W > 0) {
			hipLaunchKernelGGL(k_boot_draw, dim3((unsigned)(((int64_t)M + BLOCK - 1) / BLOCK), (unsigned)g), dim3(BLOCK), 0, st, M, in->seed, (uint32_t)(in->first + q0), d_draws);
			PANCHK(m, hipGetLastError());
			if (in->draws != nullptr) PANCHK(m, hipMemcpyAsync(in->draws + (size_t)q0 * (size_t)M, d_draws, sizeof(int32_t) * (size_t)g * (size_t)M, hipMemcpyDeviceToHost, st));
			// assemblies a workgroup takes: as many as still leave about 2 048 workgroups, 32 at the most
			const int32_t a_per = (int32_t)std::max<int64_t>(1, std::min<int64_t>(32, (int64_t)A * g * n_wc / 2048));
			const dim3 grid(n_wc, (unsigned)((A + a_per - 1) / a_per), (unsigned)g);
			if (use_lds) hipLaunchKernelGGL(k_boot_resample<true>, grid, dim3(BLOCK), sizeof(uint32_t) * (size_t)W, st, d_bits, d_draws, M, W, A, a_per, d_rows);
			else hipLaunchKernelGGL(k_boot_resample<false>, grid, dim3(BLOCK), 0, st, d_bits, d_draws, M, W, A, a_per, d_rows);
			PANCHK(m, hipGetLastError());
			if (sh.n_split > 1) PANCHK(m, hipMemsetAsync(S_g, 0, sizeof(int32_t) * (size_t)g * nn, st));
			for (int32_t q = 0; q < g; ++q)
				hipLaunchKernelGGL(k_dist_shared, dim3((unsigned)sh.n_tile * (unsigned)sh.n_split), dim3(BLOCK), 0, st, d_rows + (size_t)q * (size_t)A * (size_t)W, A, W,
				                   sh.n_chunk, sh.n_split, sh.cps, S_g + (size_t)q * nn);
			PANCHK(m, hipGetLastError());
		}
		if (diff) hipLaunchKernelGGL(k_boot_maxdiff, dim3((unsigned)std::min<size_t>((nn + BLOCK - 1) / BLOCK, 1024), (unsigned)g), dim3(BLOCK), 0, st, S_g, A, d_mx + q0);
		hipLaunchKernelGGL(k_boot_fixed, dim3((unsigned)A, (unsigned)g), dim3(BLOCK), 0, st, S_g, A, ld, diff ? 1 : 0, d_mx + q0, d_d + (size_t)q0 * (size_t)A * (size_t)ld, d_flag + q0);
		PANCHK(m, hipGetLastError());
	}
	const int rc = nj ? boot_join_queue<true>(st, d_d, A, ld, n_rep, d_label, d_aux, d_part, max_part, d_rec, rec_stride, d_flag)
	                  : boot_join_queue<false>(st, d_d, A, ld, n_rep, d_label, d_aux, d_part, max_part, d_rec, rec_stride, d_flag);
	if (rc != 0) { (void)hipStreamSynchronize(st); return rc; }
	PANCHK(m, hipMemcpyAsync(h_rec, d_rec, sizeof(int64_t) * (rec_stride * (size_t)n_rep + n_flag64), hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	const int32_t *h_flag = (const int32_t *)(h_rec + rec_stride * (size_t)n_rep);
	for (int32_t q = 0; q < n_rep; ++q)
		if (h_flag[q] != 0) return PGA_ERR_RANGE;
	out->rec = h_rec, out->n_rec = n_rec;
	return 0;
}
