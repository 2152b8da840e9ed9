// pga_pan_mantel (include/pangene_hip.h): the Mantel test of pangene mantel on the device (k_mantel.hpp).  Context-free: it runs on a
// stream of its own on the current device.  The device buffers and the page-locked results are kept from call to call in the PAN_MANTEL
// pool and only ever grow; pga_host_trim(0) gives them back.
//
// Both matrices go up once.  The identity order then goes through k_mantel_z and k_mantel_stat as a batch of one, so Z of the observed
// matrix stands in device memory before any count reads it.  The permutations follow in batches of pga_mantel_batch() orders (4 096, or
// PANGENE_MANTEL_BATCH=n up to 1 048 576): per batch k_mantel_order makes the orders, k_mantel_z adds every row block's share into Z[p]
// and k_mantel_stat counts and clears, one after the other on the one stream.  Nothing is read back between the batches and the host
// waits once, at the end (tests that ask for z_rows / ord_rows wait once more, after the first batch).
constexpr int32_t MANTEL_MAX_COL = 16384;
constexpr int32_t MANTEL_BATCH = 4096;

struct MantelBuf { enum { A, B, ORD, WORK, Z, OUT, ZROWS, N_BUF }; }; // page-locked buffer 0: out
static_assert(MantelBuf::N_BUF <= PAN_MAX_DEV, "the pool has no room for the Mantel buffers");

static size_t mantel_z_lds(int32_t N) { return ((size_t)MZ_LDS_HEAD + 4 * (size_t)((N + 3) & ~3) + 2 * (size_t)N + 15) & ~(size_t)15; }

extern "C" int32_t pga_mantel_batch(void) { return (int32_t)pan_env("PANGENE_MANTEL_BATCH", MANTEL_BATCH, 1 << 20); }

extern "C" int pga_pan_mantel(const pga_mantel_in_t *in, pga_mantel_out_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	memset(out, 0, sizeof(*out));
	if (in == nullptr || in->a == nullptr || in->b == nullptr) return PGA_ERR_ARG;
	const int32_t N = in->n, n = in->n_perm;
	if (N < 1 || n < 0 || in->max_a < 0 || in->max_b < 0) return PGA_ERR_ARG;
	if (N > MANTEL_MAX_COL || n > PAN_MAX_PERM) return PGA_ERR_RANGE; // (before anything is launched)
	if ((unsigned __int128)((uint64_t)in->max_a * (uint64_t)in->max_b) * ((uint64_t)N * (uint64_t)(N - 1)) >= (unsigned __int128)1 << 62) return PGA_ERR_ARG; // the caller's shifts are too small
	PermBatches b(n, pga_mantel_batch(), N <= MANTEL_ORDER_LDS_N);
	const int32_t B = b.B;
	const bool tests = in->z_rows != nullptr;
	const size_t nn = (size_t)N * (size_t)N, z_lds = mantel_z_lds(N);
	PanDev &m = g_pan[PAN_MANTEL];
	std::lock_guard<std::mutex> lk(m.mu);
	int64_t *h_out = m.get_host<int64_t>(0, MT_N_OUT);
	PANMEM(h_out);
	hipStream_t st;
	PANCHK(m, m.stream(&st));
	int32_t *d_a = m.get<int32_t>(MantelBuf::A, nn), *d_b = m.get<int32_t>(MantelBuf::B, nn);
	uint16_t *d_ord = m.get<uint16_t>(MantelBuf::ORD, (size_t)B * (size_t)N);
	uint16_t *d_work = m.get<uint16_t>(MantelBuf::WORK, b.work((size_t)N));
	unsigned long long *d_z = m.get<unsigned long long>(MantelBuf::Z, (size_t)B);
	long long *d_out = m.get<long long>(MantelBuf::OUT, MT_N_OUT);
	long long *d_zrows = m.get<long long>(MantelBuf::ZROWS, tests ? (size_t)B : 1);
	PANMEM(d_a); PANMEM(d_b); PANMEM(d_ord); PANMEM(d_work); PANMEM(d_z); PANMEM(d_out); PANMEM(d_zrows);
	if (z_lds > 65536) PANCHK(m, hipFuncSetAttribute((const void *)k_mantel_z, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mantel_z_lds(MANTEL_MAX_COL)));
	PANCHK(m, hipMemcpyAsync(d_a, in->a, sizeof(int32_t) * nn, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemcpyAsync(d_b, in->b, sizeof(int32_t) * nn, hipMemcpyHostToDevice, st));
	PANCHK(m, hipMemsetAsync(d_out, 0, sizeof(long long) * MT_N_OUT, st));
	PANCHK(m, hipMemsetAsync(d_z, 0, sizeof(unsigned long long) * (size_t)B, st));
	const unsigned row_blocks = (unsigned)((N - 1 + MZ_ROWS - 1) / MZ_ROWS); // 0 at N = 1: no pair, Z = 0 without a launch
	auto orders = [&](uint32_t p0, int32_t nb, bool identity) {
		perm_launch(b.lds, k_mantel_order<true>, k_mantel_order<false>, nb, st, N, in->seed, p0, nb, identity, d_work, d_ord);
	};
	// the observed matrix: a batch of one with the identity order
	orders(0, 1, true);
	if (row_blocks) hipLaunchKernelGGL(k_mantel_z, dim3(1, row_blocks), dim3(BLOCK), z_lds, st, d_a, d_b, d_ord, N, d_z);
	hipLaunchKernelGGL(k_mantel_stat, dim3(1), dim3(BLOCK), 0, st, d_z, 1, true, d_out, (long long *)nullptr);
	PANCHK(m, hipGetLastError());
	for (; b.more(); b.next()) {
		const int32_t nb = b.nb();
		const bool first = b.first();
		orders(b.p0(), nb, false);
		if (row_blocks) hipLaunchKernelGGL(k_mantel_z, dim3((unsigned)nb, row_blocks), dim3(BLOCK), z_lds, st, d_a, d_b, d_ord, N, d_z);
		hipLaunchKernelGGL(k_mantel_stat, dim3((unsigned)((nb + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, st, d_z, nb, false, d_out, first && tests ? d_zrows : (long long *)nullptr);
		PANCHK(m, hipGetLastError());
		if (first && (tests || in->ord_rows != nullptr)) { // tests only: the first batch's Z_p and orders
			if (in->z_rows != nullptr) PANCHK(m, hipMemcpyAsync(in->z_rows, d_zrows, sizeof(int64_t) * (size_t)nb, hipMemcpyDeviceToHost, st));
			if (in->ord_rows != nullptr) PANCHK(m, hipMemcpyAsync(in->ord_rows, d_ord, sizeof(uint16_t) * (size_t)nb * (size_t)N, hipMemcpyDeviceToHost, st));
			PANCHK(m, hipStreamSynchronize(st));
		}
	}
	PANCHK(m, hipMemcpyAsync(h_out, d_out, sizeof(int64_t) * MT_N_OUT, hipMemcpyDeviceToHost, st));
	PANCHK(m, hipStreamSynchronize(st));
	out->z = h_out[MT_Z], out->n_ge = h_out[MT_GE], out->n_le = h_out[MT_LE];
	return 0;
}
