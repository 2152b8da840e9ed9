// pga_pan_permanova (include/pangene_hip.h): the two-group PERMANOVA of pangene permanova on the device (k_permanova.hpp).  Context-free:
// it runs on a stream of its own on the current device.  The device buffers and the page-locked results are kept from call to call in the
// PAN_PERMANOVA pool and only ever grow; pga_host_trim(0) gives them back.
//
// The matrix goes up once and k_perma_prep turns it into the digit planes, r and T.  The observed label row then goes through
// k_perma_quad and k_perma_stat as a one-row batch, so A and B of the observed row stand in device memory before any count reads them.
// The permutations follow in batches of pga_permanova_batch() rows (16 384, or PANGENE_PERMA_BATCH=n up to 1 048 576): per batch
// k_trait_perm makes the bit rows, k_perma_quad adds every (column tile, plane) share into A[p] and k_perma_stat counts and clears, one
// after the other on the one stream.  Nothing is read back between the batches and the host waits once, at the end (tests that ask for
// a_rows / b_rows / perm_rows wait once more, after the first batch).  Every plane is launched: telling an all-zero plane apart would
// take a read of its own.
constexpr int32_t PERMA_MAX_COL = 16384;
constexpr int32_t PERMA_BATCH = 16384;

struct PermaBuf { enum { Q, PL, R, LABEL, ROWS, WORK, A, OUT, AROWS, BROWS, N_BUF }; }; // page-locked buffer 0: out; 1, 2: a_rows, b_rows (tests)
static_assert(PermaBuf::N_BUF <= PAN_MAX_DEV, "the pool has no room for the PERMANOVA buffers");

extern "C" int32_t pga_permanova_batch(void) { return (int32_t)pan_env("PANGENE_PERMA_BATCH", PERMA_BATCH, 1 << 20); }

extern "C" int pga_pan_permanova(const pga_permanova_in_t *in, pga_permanova_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	memset(out, 0, sizeof(*out));
	if (in == nullptr || in->q == nullptr || in->label == nullptr) return PGA_ERR_ARG;
	const int32_t N = in->n, n = in->n_perm, n1 = in->n1;
	if (N < 1 || n < 0 || in->shift < 0 || in->shift > 30 || in->q_max < 0 || n1 < 0 || n1 > N) return PGA_ERR_ARG;
	if (N > PERMA_MAX_COL || n > PAN_MAX_PERM) return PGA_ERR_RANGE; // (before anything is launched)
	const uint64_t e_max = (uint64_t)(in->q_max >> in->shift), w_max = e_max * e_max;
	if ((unsigned __int128)w_max * (uint64_t)N * (uint64_t)(N - 1) >= (unsigned __int128)1 << 62) return PGA_ERR_ARG; // the caller's shift is too small
	int32_t D = 1;
	for (uint64_t cap = 127; cap < w_max; cap = cap * 256 + 127) ++D; // 127 (256^D - 1) / 255, the largest value D balanced digits hold
	const int32_t W = (N + 31) / 32, Np = (N + PM_TILE - 1) / PM_TILE * PM_TILE;
	PermBatches b(n, pga_permanova_batch(), W <= TRAIT_PERM_LDS_W);
	const int32_t B = b.B;
	const bool tests = in->a_rows != nullptr || in->b_rows != nullptr;
	PanDev &m = g_pan[PAN_PERMANOVA];
	std::lock_guard<std::mutex> lk(m.mu);
	int64_t *h_out = m.get_host<int64_t>(0, PM_N_OUT);
	PANMEM(h_out);
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	int32_t *d_q = m.get<int32_t>(PermaBuf::Q, (size_t)N * (size_t)N);
	int8_t *d_pl = m.get<int8_t>(PermaBuf::PL, (size_t)D * (size_t)Np * (size_t)Np);
	long long *d_r = m.get<long long>(PermaBuf::R, (size_t)W * 32); // (k_perma_stat indexes it by bit position)
	uint32_t *d_label = m.get<uint32_t>(PermaBuf::LABEL, (size_t)W), *d_rows = m.get<uint32_t>(PermaBuf::ROWS, (size_t)B * (size_t)W);
	uint32_t *d_work = m.get<uint32_t>(PermaBuf::WORK, b.work((size_t)W));
	unsigned long long *d_a = m.get<unsigned long long>(PermaBuf::A, (size_t)B);
	long long *d_out = m.get<long long>(PermaBuf::OUT, PM_N_OUT);
	long long *d_arows = m.get<long long>(PermaBuf::AROWS, tests ? (size_t)B : 1), *d_brows = m.get<long long>(PermaBuf::BROWS, tests ? (size_t)B : 1);
	PANMEM(d_q); PANMEM(d_pl); PANMEM(d_r); PANMEM(d_label); PANMEM(d_rows); PANMEM(d_work); PANMEM(d_a); PANMEM(d_out); PANMEM(d_arows); PANMEM(d_brows);
	PANCHK(m, hipMemcpyAsync(d_q, in->q, sizeof(int32_t) * (size_t)N * (size_t)N, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_label, in->label, sizeof(uint32_t) * (size_t)W, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_out, 0, sizeof(long long) * PM_N_OUT, st));
	PANCHK(m, hipMemsetAsync(d_a, 0, sizeof(unsigned long long) * (size_t)B, st));
	const unsigned col_tiles = (unsigned)(Np / PM_TILE), stat_rows = BLOCK / PM_ROW_LANES;
	hipLaunchKernelGGL(k_perma_prep, dim3((unsigned)Np), dim3(BLOCK), 0, st, d_q, N, Np, in->shift, D, d_pl, d_r, (unsigned long long *)d_out);
	// the observed row: a batch of one
	hipLaunchKernelGGL(k_perma_quad, dim3(col_tiles, 1, (unsigned)D), dim3(BLOCK), 0, st, d_label, d_pl, 1, W, Np, d_a);
	hipLaunchKernelGGL(k_perma_stat, dim3(1), dim3(BLOCK), 0, st, d_label, d_r, 1, W, N, n1, true, d_a, d_out, (long long *)nullptr, (long long *)nullptr);
	PANCHK(m, hipGetLastError());
	for (; b.more(); b.next()) {
		const int32_t nb = b.nb();
		const bool first = b.first();
		perm_launch(b.lds, k_trait_perm<true>, k_trait_perm<false>, nb, st, d_label, N, W, in->seed, b.p0(), nb, d_work, d_rows);
		hipLaunchKernelGGL(k_perma_quad, dim3(col_tiles, (unsigned)((nb + PM_TILE - 1) / PM_TILE), (unsigned)D), dim3(BLOCK), 0, st, d_rows, d_pl, nb, W, Np, d_a);
		hipLaunchKernelGGL(k_perma_stat, dim3((unsigned)((nb + stat_rows - 1) / stat_rows)), dim3(BLOCK), 0, st, d_rows, d_r, nb, W, N, n1, false, d_a, d_out,
		                   first && tests ? d_arows : (long long *)nullptr, first && tests ? d_brows : (long long *)nullptr);
		PANCHK(m, hipGetLastError());
		if (first && (tests || in->perm_rows != nullptr)) { // tests only: the first batch's A_p, B_p and label rows
			if (in->a_rows != nullptr) PANCHK(m, hipMemcpyAsync(in->a_rows, d_arows, sizeof(int64_t) * (size_t)nb, hipMemcpyDeviceToHost, st));
			if (in->b_rows != nullptr) PANCHK(m, hipMemcpyAsync(in->b_rows, d_brows, sizeof(int64_t) * (size_t)nb, hipMemcpyDeviceToHost, st));
			if (in->perm_rows != nullptr) PANCHK(m, hipMemcpyAsync(in->perm_rows, d_rows, sizeof(uint32_t) * (size_t)nb * (size_t)W, hipMemcpyDeviceToHost, st));
			PANCHK(m, hipStreamSynchronize(st));
		}
	}
	PANCHK(m, hipMemcpyAsync(h_out, d_out, sizeof(int64_t) * PM_N_OUT, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	out->t = h_out[PM_T], out->a = h_out[PM_A], out->b = h_out[PM_B], out->k = h_out[PM_K];
	return 0;
}
