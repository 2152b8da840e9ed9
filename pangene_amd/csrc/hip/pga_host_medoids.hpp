// pga_pan_medoids (include/pangene_hip.h): k-medoids over a fixed-point distance matrix on the device (k_medoids.hpp).  Context-free like
// pga_pan_join: a stream of its own on the current device, buffers kept from call to call in the PAN_MEDOIDS pool.  The matrix goes up
// once and stays for the whole call.  BUILD is queued without reading anything back.  The swap iterations are queued in chunks of
// med_batch(); after a chunk the host reads the status and the chunk's records in one small copy -- that is the only wait of the loop,
// and every kernel of an iteration that comes after convergence returns at once.  The finish is queued behind the loop and everything
// else comes back in one copy.

struct MedBuf { enum { Q, D, DS, NN, MED, ISMED, GAIN, SLOT, REMOVAL, CNT, ACC, PLUS, PERM, STAT, OUT, N_BUF }; };
static_assert(MedBuf::N_BUF <= PAN_MAX_DEV, "the pool has no room for the medoid buffers");

// iterations the host queues between two reads of the status: 8, or PANGENE_MEDOIDS_BATCH (tests)
static int32_t med_batch() { return (int32_t)pan_env("PANGENE_MEDOIDS_BATCH", 8, 1024); }

// The launch shape of the row walk over n columns: tiles of BLOCK candidates x chunks of `rows` permuted rows.  Where the tiles alone
// are fewer than MED_WANT_WG workgroups the rows are cut into as many chunks as it takes to get there, MED_MIN_ROWS rows a chunk at the
// least: n = 2 000 gives 8 x 125 workgroups of 16 rows, n = 10 000 gives 40 x 52 of 193.  PANGENE_MEDOIDS_ROWS fixes the rows (tests).
struct MedShape { int32_t n_tile, rows, n_chunk; };
static MedShape med_shape(int32_t n)
{
	MedShape s;
	s.n_tile = (n + BLOCK - 1) / BLOCK;
	const int32_t want = std::max(1, (MED_WANT_WG + s.n_tile - 1) / s.n_tile);
	s.rows = std::max(MED_MIN_ROWS, (n + want - 1) / want);
	s.rows = (int32_t)pan_env("PANGENE_MEDOIDS_ROWS", s.rows, n);
	s.n_chunk = (n + s.rows - 1) / s.rows;
	return s;
}

static std::vector<int64_t> g_med_rec; // the records of the last call (guarded by the pool's lock)

extern "C" int pga_pan_medoids(const pga_medoids_in_t *in, pga_medoids_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	memset(out, 0, sizeof(*out));
	if (in == nullptr || in->q == nullptr || in->n < 3 || in->k < 2 || in->k > in->n - 1 || in->max_iter < 0) return PGA_ERR_ARG;
	const int32_t n = in->n, k = in->k;
	if (n > 65535 || k > MED_MAX_K) return PGA_ERR_RANGE;
	const int32_t ld = (n + 3) & ~3, batch = med_batch();
	const MedShape sh = med_shape(n);
	const unsigned n_grid = (unsigned)((n + BLOCK - 1) / BLOCK);
	PanDev &m = g_pan[PAN_MEDOIDS];
	std::lock_guard<std::mutex> lk(m.mu);
	// page-locked: 0 = the status and a chunk's records, 1 = everything else: td, sums, BUILD's records, then the int32 arrays
	const size_t n64 = 1 + (size_t)n * (size_t)k + 3 * (size_t)k, n32 = 2 * (size_t)k + 2 * (size_t)n;
	int64_t *h_stat = m.get_host<int64_t>(0, 1 + 3 * (size_t)batch), *h_out = m.get_host<int64_t>(1, n64 + (n32 + 1) / 2);
	PANMEM(h_stat); PANMEM(h_out);
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	int32_t *d_q = m.get<int32_t>(MedBuf::Q, (size_t)n * (size_t)ld), *d_D = m.get<int32_t>(MedBuf::D, (size_t)n), *d_DS = m.get<int32_t>(MedBuf::DS, (size_t)n);
	uint16_t *d_NN = m.get<uint16_t>(MedBuf::NN, (size_t)n);
	int32_t *d_med = m.get<int32_t>(MedBuf::MED, (size_t)k), *d_ismed = m.get<int32_t>(MedBuf::ISMED, (size_t)n), *d_slot = m.get<int32_t>(MedBuf::SLOT, (size_t)n);
	long long *d_gain = m.get<long long>(MedBuf::GAIN, (size_t)n), *d_removal = m.get<long long>(MedBuf::REMOVAL, (size_t)k);
	int32_t *d_cnt = m.get<int32_t>(MedBuf::CNT, 2 * (size_t)k); // cnt[k], fill[k]
	long long *d_acc = m.get<long long>(MedBuf::ACC, (size_t)n * (size_t)k), *d_plus = m.get<long long>(MedBuf::PLUS, (size_t)n);
	int32_t *d_perm = m.get<int32_t>(MedBuf::PERM, (size_t)n);
	long long *d_stat = m.get<long long>(MedBuf::STAT, 1 + 3 * (size_t)batch), *d_out = m.get<long long>(MedBuf::OUT, n64 + (n32 + 1) / 2);
	PANMEM(d_q); PANMEM(d_D); PANMEM(d_DS); PANMEM(d_NN); PANMEM(d_med); PANMEM(d_ismed); PANMEM(d_slot); PANMEM(d_gain); PANMEM(d_removal); PANMEM(d_cnt);
	PANMEM(d_acc); PANMEM(d_plus); PANMEM(d_perm); PANMEM(d_stat); PANMEM(d_out);
	int32_t *d_fill = d_cnt + k;
	MedStat *d_status = (MedStat *)d_stat;
	long long *d_td = d_out, *d_sums = d_out + 1, *d_rec0 = d_sums + (size_t)n * (size_t)k;
	int32_t *d_medoid = (int32_t *)(d_out + n64), *d_size = d_medoid + k, *d_label = d_size + k, *d_dist = d_label + n;

	if (ld == n) PANCHK(m, hipMemcpyAsync(d_q, in->q, sizeof(int32_t) * (size_t)n * (size_t)n, hipMemcpyHostToDevice, st));
	else PANCHK(m, hipMemcpy2DAsync(d_q, sizeof(int32_t) * (size_t)ld, in->q, sizeof(int32_t) * (size_t)n, sizeof(int32_t) * (size_t)n, (size_t)n, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetD32Async((hipDeviceptr_t)d_D, MED_LIMIT, (size_t)n, st));
	PANCHK(m, hipMemsetAsync(d_ismed, 0xff, sizeof(int32_t) * (size_t)n, st));
	PANCHK(m, hipMemsetAsync(d_removal, 0, sizeof(long long) * (size_t)k, st));
	PANCHK(m, hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * 2 * (size_t)k, st));
	PANCHK(m, hipMemsetAsync(d_acc, 0, sizeof(long long) * (size_t)n * (size_t)k, st));
	PANCHK(m, hipMemsetAsync(d_plus, 0, sizeof(long long) * (size_t)n, st));
	PANCHK(m, hipMemsetAsync(d_stat, 0, sizeof(long long), st));
	for (int32_t s = 0; s < k; ++s) {
		hipLaunchKernelGGL(k_med_gain, dim3((unsigned)n), dim3(BLOCK), 0, st, d_q, n, ld, d_D, d_ismed, d_gain);
		hipLaunchKernelGGL(k_med_build_pick, dim3(1), dim3(BLOCK), 0, st, d_q, n, ld, s, d_gain, d_D, d_med, d_ismed, d_rec0);
		if ((s & 255) == 255) PANCHK(m, hipGetLastError());
	}
	hipLaunchKernelGGL(k_med_assign, dim3(n_grid), dim3(BLOCK), 0, st, d_q, n, ld, k, d_med, d_D, d_DS, d_NN, d_removal, d_cnt, (const MedStat *)nullptr);
	hipLaunchKernelGGL(k_med_scatter, dim3(n_grid), dim3(BLOCK), 0, st, n, k, d_NN, d_cnt, d_fill, d_perm, (const MedStat *)nullptr);
	PANCHK(m, hipGetLastError());

	g_med_rec.assign(3 * (size_t)k, 0);
	int32_t n_swap = 0, done = 0;
	for (int32_t it = 0; it < in->max_iter && !done; ) {
		const int32_t nb = std::min(batch, in->max_iter - it);
		for (int32_t b = 0; b < nb; ++b) {
			hipLaunchKernelGGL(k_med_swap, dim3((unsigned)sh.n_tile, (unsigned)sh.n_chunk), dim3(BLOCK), 0, st, d_q, n, ld, sh.rows, d_perm, d_NN, d_D, d_DS, d_acc, d_plus, d_status);
			hipLaunchKernelGGL(k_med_best, dim3(n_grid), dim3(BLOCK), 0, st, n, k, d_med, d_ismed, d_removal, d_acc, d_plus, d_gain, d_slot, d_status);
			hipLaunchKernelGGL(k_med_pick, dim3(1), dim3(BLOCK), 0, st, n, k, d_gain, d_slot, d_med, d_ismed, d_removal, d_cnt, d_fill, d_stat + 1, n_swap, d_status);
			hipLaunchKernelGGL(k_med_assign, dim3(n_grid), dim3(BLOCK), 0, st, d_q, n, ld, k, d_med, d_D, d_DS, d_NN, d_removal, d_cnt, d_status);
			hipLaunchKernelGGL(k_med_scatter, dim3(n_grid), dim3(BLOCK), 0, st, n, k, d_NN, d_cnt, d_fill, d_perm, d_status);
		}
		PANCHK(m, hipGetLastError());
		PANCHK(m, hipMemcpyAsync(h_stat, d_stat, sizeof(int64_t) * (1 + 3 * (size_t)nb), hipMemcpyDeviceToHost, st));
		PANCHK(m, hipStreamSynchronize(st));
		const MedStat now = *(const MedStat *)h_stat;
		if (now.n_swap < n_swap || now.n_swap - n_swap > nb) return PGA_ERR_INVARIANT;
		g_med_rec.insert(g_med_rec.end(), h_stat + 1, h_stat + 1 + 3 * (size_t)(now.n_swap - n_swap));
		n_swap = now.n_swap, done = now.done, it += nb;
	}

	hipLaunchKernelGGL(k_med_rank, dim3(1), dim3(BLOCK), 0, st, k, d_med, d_medoid, d_ismed, d_cnt, d_fill, d_td);
	hipLaunchKernelGGL(k_med_label, dim3(n_grid), dim3(BLOCK), 0, st, d_q, n, ld, k, d_medoid, d_ismed, d_label, d_dist, d_NN, d_cnt, d_td);
	hipLaunchKernelGGL(k_med_scatter, dim3(n_grid), dim3(BLOCK), 0, st, n, k, d_NN, d_cnt, d_fill, d_perm, (const MedStat *)nullptr);
	hipLaunchKernelGGL(k_med_sums, dim3((unsigned)sh.n_tile, (unsigned)sh.n_chunk), dim3(BLOCK), 0, st, d_q, n, ld, sh.rows, d_perm, d_NN, d_acc);
	hipLaunchKernelGGL(k_med_out, dim3(n_grid), dim3(BLOCK), 0, st, n, k, d_acc, d_cnt, d_sums, d_size);
	PANCHK(m, hipGetLastError());
	PANCHK(m, hipMemcpyAsync(h_out, d_out, sizeof(int64_t) * (n64 + (n32 + 1) / 2), hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	std::copy(h_out + 1 + (size_t)n * (size_t)k, h_out + n64, g_med_rec.begin());
	const int32_t *h32 = (const int32_t *)(h_out + n64);
	out->medoid = h32, out->size = h32 + k, out->label = h32 + 2 * (size_t)k, out->dist = h32 + 2 * (size_t)k + n;
	out->sums = h_out + 1, out->td = h_out[0];
	out->rec = g_med_rec.data(), out->n_rec = k + n_swap, out->n_swap = n_swap, out->converged = done;
	return 0;
}
