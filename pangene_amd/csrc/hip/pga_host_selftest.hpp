// pga_host_selftest.hpp -- self-tests of the device primitives and the counter calibration kernels (tests/, profiles/tools/calibrate.py).
// Host side of the device ABI (include/pangene_hip.h); included by pga_backend.hip (one translation unit), in this order.
#pragma once


// ------------------------------------------------------------------------------------------------
// self-test hooks for the device primitives (tests/test_hip_parity.py: test_device_primitives, test_radix_sort_key_widths): sort / scan arbitrary host data
// ------------------------------------------------------------------------------------------------
extern "C" int pga_selftest_sort(uint64_t *keys, uint32_t *vals, int64_t n, int32_t n_bits)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PGA_ERR_NO_DEVICE;
	uint64_t *ka, *kb; uint32_t *va, *vb, *table; int32_t *tile;
	HIPCHK(hipMalloc((void **)&ka, sizeof(uint64_t) * (size_t)(n + 1))); HIPCHK(hipMalloc((void **)&kb, sizeof(uint64_t) * (size_t)(n + 1)));
	HIPCHK(hipMalloc((void **)&va, sizeof(uint32_t) * (size_t)(n + 1))); HIPCHK(hipMalloc((void **)&vb, sizeof(uint32_t) * (size_t)(n + 1)));
	HIPCHK(hipMalloc((void **)&table, sizeof(uint32_t) * (size_t)(rs_table_len(n) + 1)));
	HIPCHK(hipMalloc((void **)&tile, tile_buf_bytes(n)));
	HIPCHK(hipMemcpy(ka, keys, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(va, vals, sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice));
	RadixBufs b = { kb, vb, table, tile };
	uint64_t *kr; uint32_t *vr;
	device_radix_sort(ka, va, n, n_bits, b, &kr, &vr, 0);
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(keys, kr, sizeof(uint64_t) * (size_t)n, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(vals, vr, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
	(void)hipFree(ka); (void)hipFree(kb); (void)hipFree(va); (void)hipFree(vb); (void)hipFree(table); (void)hipFree(tile);
	return 0;
}

// cross-shard arc merge on host data: `gathered` holds W slots of slot_sz entries (count[r] valid, sorted by x, unique keys)
extern "C" int pga_selftest_merge(const pga_arc_part_t *gathered, const int64_t *count, int32_t W, int64_t slot_sz, pga_arc_part_t *out, int64_t *n_out)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PGA_ERR_NO_DEVICE;
	pga_ctx c; // a bare context: stream, counters, pool
	HIPCHK(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
	TRY(dalloc(&c, &c.dcnt, 16)); TRY(dalloc_commit(&c));
	HIPCHK(hipHostMalloc((void **)&c.h_cnt, 16 * sizeof(int64_t), hipHostMallocDefault));
	pga_arc_part_t *dg = nullptr, *res = nullptr;
	HIPCHK(hipMalloc((void **)&dg, sizeof(pga_arc_part_t) * (size_t)(W * slot_sz + 1)));
	HIPCHK(hipMemcpy(dg, gathered, sizeof(pga_arc_part_t) * (size_t)(W * slot_sz), hipMemcpyHostToDevice));
	int rc = pga_arc_merge(&c, dg, count, W, slot_sz, &res, n_out);
	if (rc == 0 && *n_out) rc = hipMemcpyAsync(out, res, sizeof(pga_arc_part_t) * (size_t)*n_out, hipMemcpyDeviceToHost, c.st) == hipSuccess ? 0 : PGA_ERR_NO_DEVICE;
	(void)hipStreamSynchronize(c.st);
	(void)hipFree(dg); (void)hipFree(c.dcnt); (void)hipHostFree(c.h_cnt);
	c.pool.release();
	(void)hipStreamDestroy(c.st);
	return rc;
}

// ------------------------------------------------------------------------------------------------
// Calibration of the rocprofv3 memory counters (profiles/tools/calibrate.py): kernels with KNOWN byte counts in the access patterns the
// path's kernels use -- coalesced streams of 4 and 16 bytes per lane, 4- and 16-byte gathers / scatters through a permutation (inside
// windows of `window` items, or over the whole array) -- so that FETCH_SIZE / WRITE_SIZE can be turned into bytes per pattern instead
// of by one factor for everything (MI355X_MICROARCH.md calibrates the factor 2 of FETCH_SIZE for wide coalesced reads only).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t cal_perm(int64_t i, int64_t n, int64_t window) // a bijection of [0, n) that permutes inside windows (a power of two)
{
	const int64_t base = i & ~(window - 1), span = base + window <= n ? window : 0; // (the last, partial window stays in place)
	return span ? base + (((i - base) * 40503 + 12345) & (window - 1)) : i;
}
__global__ __launch_bounds__(BLOCK) void k_cal_read16(const int4 *__restrict__ src, int64_t n, int32_t *sink)
{
	int acc = 0;
	for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) { const int4 v = src[i]; acc ^= v.x ^ v.y ^ v.z ^ v.w; }
	if (acc == 0x7fffffff) sink[0] = acc;
}
__global__ __launch_bounds__(BLOCK) void k_cal_read4(const int32_t *__restrict__ src, int64_t n, int32_t *sink)
{
	int acc = 0;
	for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) acc ^= src[i];
	if (acc == 0x7fffffff) sink[0] = acc;
}
__global__ __launch_bounds__(BLOCK) void k_cal_gather4(const int32_t *__restrict__ src, int64_t n, int64_t window, int32_t *sink)
{
	int acc = 0;
	for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) acc ^= src[cal_perm(i, n, window)];
	if (acc == 0x7fffffff) sink[0] = acc;
}
__global__ __launch_bounds__(BLOCK) void k_cal_gather16(const int4 *__restrict__ src, int64_t n, int64_t window, int32_t *sink)
{
	int acc = 0;
	for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) { const int4 v = src[cal_perm(i, n, window)]; acc ^= v.x ^ v.w; }
	if (acc == 0x7fffffff) sink[0] = acc;
}
__global__ __launch_bounds__(BLOCK) void k_cal_write16(int4 *__restrict__ dst, int64_t n)
{
	for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) dst[i] = make_int4((int)i, 1, 2, 3);
}
__global__ __launch_bounds__(BLOCK) void k_cal_write4(int32_t *__restrict__ dst, int64_t n)
{
	for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) dst[i] = (int)i;
}
__global__ __launch_bounds__(BLOCK) void k_cal_scatter4(int32_t *__restrict__ dst, int64_t n, int64_t window)
{
	for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) dst[cal_perm(i, n, window)] = (int)i;
}
__global__ __launch_bounds__(BLOCK) void k_cal_scatter16(int4 *__restrict__ dst, int64_t n, int64_t window)
{
	for (int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * BLOCK) dst[cal_perm(i, n, window)] = make_int4((int)i, 1, 2, 3);
}

// runs every pattern once over n items (n * 16 bytes must be past the 256 MiB Infinity Cache to mean anything); the names of the
// kernels carry the pattern, the caller knows the bytes: read16 16 n, read4 4 n, gather4 4 n, gather16 16 n, write16 16 n,
// write4 4 n, scatter4 4 n, scatter16 16 n.  window: a power of two (a genome's worth of items), or 0 = the whole array (rounded down).
extern "C" int pga_selftest_traffic(int64_t n, int64_t window)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PGA_ERR_NO_DEVICE;
	if (n < 1024) return PGA_ERR_ARG;
	if (window <= 0) { window = 1; while (window * 2 <= n) window *= 2; }
	if (window & (window - 1)) return PGA_ERR_ARG;
	int4 *a = nullptr, *b = nullptr; int32_t *sink = nullptr;
	HIPCHK(hipMalloc((void **)&a, sizeof(int4) * (size_t)n)); HIPCHK(hipMalloc((void **)&b, sizeof(int4) * (size_t)n)); HIPCHK(hipMalloc((void **)&sink, 256));
	HIPCHK(hipMemset(a, 1, sizeof(int4) * (size_t)n)); HIPCHK(hipMemset(b, 2, sizeof(int4) * (size_t)n));
	HIPCHK(hipDeviceSynchronize());
	const unsigned grid = (unsigned)std::min<int64_t>((n + BLOCK - 1) / BLOCK, (int64_t)256 * 64);
	hipLaunchKernelGGL(k_cal_read16, dim3(grid), dim3(BLOCK), 0, 0, (const int4 *)a, n, sink);
	hipLaunchKernelGGL(k_cal_read4, dim3(grid), dim3(BLOCK), 0, 0, (const int32_t *)b, n, sink);
	hipLaunchKernelGGL(k_cal_gather4, dim3(grid), dim3(BLOCK), 0, 0, (const int32_t *)a, n, window, sink);
	hipLaunchKernelGGL(k_cal_gather16, dim3(grid), dim3(BLOCK), 0, 0, (const int4 *)b, n, window, sink);
	hipLaunchKernelGGL(k_cal_write16, dim3(grid), dim3(BLOCK), 0, 0, a, n);
	hipLaunchKernelGGL(k_cal_write4, dim3(grid), dim3(BLOCK), 0, 0, (int32_t *)b, n);
	hipLaunchKernelGGL(k_cal_scatter4, dim3(grid), dim3(BLOCK), 0, 0, (int32_t *)a, n, window);
	hipLaunchKernelGGL(k_cal_scatter16, dim3(grid), dim3(BLOCK), 0, 0, b, n, window);
	HIPCHK(hipDeviceSynchronize());
	(void)hipFree(a); (void)hipFree(b); (void)hipFree(sink);
	return 0;
}

// mode 0: exclusive sum; 1: exclusive max (identity -1); 2: segmented inclusive max with seg[]
extern "C" int pga_selftest_scan(const int32_t *in, const int32_t *seg, int32_t *out, int64_t n, int32_t mode)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PGA_ERR_NO_DEVICE;
	int32_t *di, *ds, *dout; int64_t *tile;
	HIPCHK(hipMalloc((void **)&di, sizeof(int32_t) * (size_t)(n + 1))); HIPCHK(hipMalloc((void **)&ds, sizeof(int32_t) * (size_t)(n + 1)));
	HIPCHK(hipMalloc((void **)&dout, sizeof(int32_t) * (size_t)(n + 1))); HIPCHK(hipMalloc((void **)&tile, sizeof(int64_t) * (size_t)(scan_tiles(n) + 8)));
	HIPCHK(hipMemcpy(di, in, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
	if (seg) HIPCHK(hipMemcpy(ds, seg, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
	if (mode == 0) device_scan<I32>(InI32{di}, OutExclI32{dout}, n, (I32 *)tile, OpSum{}, I32{0}, 0);
	else if (mode == 1) device_scan<I32>(InI32{di}, OutExclI32{dout}, n, (I32 *)tile, OpMax{}, I32{-1}, 0);
	else device_scan<SegMax>(InSegMax{ds, di}, OutSegMax{dout}, n, (SegMax *)tile, OpSegMax{}, SegMax{SEG_EMPTY, 0}, 0);
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(out, dout, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
	(void)hipFree(di); (void)hipFree(ds); (void)hipFree(dout); (void)hipFree(tile);
	return 0;
}

// what pga_begin left, on whichever route made it (tests/test_stage_a_gpu.py, tests/support/stage_a_direct.py): the packed records, the raw
// flag words with the values of the internal bits, fidx / gnm / yperm / headpos -- the arrays EVERY route writes (the LDS routes write neither
// c->cs, ce, cds, offx, rk, pm as planes nor sdom / pdom / pdom0) -- and which route it was.  Reads only; not part of pangene_hip.h.
typedef struct {
	int32_t *recA, *recB, *recC;   /* [4 N] each, X order: {cs, seg, ce, pm} {rk, gid, cds, pid} {rank, n_exon, off_exon, score_ori} */
	uint32_t *flags;               /* [N] the raw flag words, X order */
	int32_t *fidx, *gnm, *yperm;   /* [N] */
	int32_t *headpos;              /* [n_genome + 1] */
	uint32_t f_head, f_multi, f_cstie;          /* out: the values of the internal bits */
	int32_t route;                 /* out: 0 global radix, 1 per-genome LDS sort, 2 contig bins */
	int32_t n_unit[3];             /* out: route 1: gs_n[0..2]; route 2: {bin_n_small, bin_n_big, 0}; route 0: zeros */
	int32_t n_cu;
} pga_selftest_stage_a_t;
extern "C" int pga_selftest_stage_a(pga_ctx_t *c, pga_selftest_stage_a_t *out) // after pga_begin: waits for the stream, copies; any pointer may be NULL
{
	if (c == nullptr || out == nullptr) return PGA_ERR_ARG;
	TRY(sync_st(c));
	const size_t N = (size_t)c->N, GL = (size_t)c->n_genome;
	auto fetch = [&](void *dst, const void *src, size_t bytes) { return (dst == nullptr || bytes == 0 || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess) ? 0 : PGA_ERR_NO_DEVICE; };
	TRY(fetch(out->recA, c->recA, sizeof(int4) * N)); TRY(fetch(out->recB, c->recB, sizeof(int4) * N)); TRY(fetch(out->recC, c->recC, sizeof(int4) * N));
	TRY(fetch(out->flags, c->flags, sizeof(uint32_t) * N));
	TRY(fetch(out->fidx, c->fidx, sizeof(int32_t) * N)); TRY(fetch(out->gnm, c->gnm, sizeof(int32_t) * N)); TRY(fetch(out->yperm, c->yperm, sizeof(int32_t) * N));
	if (N) TRY(fetch(out->headpos, c->headpos, sizeof(int32_t) * (GL + 1))); // (a shard without hits: pga_begin leaves before anybody writes it)
	out->f_head = F_HEAD, out->f_multi = F_MULTI, out->f_cstie = F_CSTIE;
	out->route = c->bin_on ? 2 : c->gs_ok ? 1 : 0, out->n_cu = c->n_cu;
	for (int k = 0; k < 3; ++k) out->n_unit[k] = out->route == 1 ? c->gs_n[k] : 0;
	if (out->route == 2) out->n_unit[0] = c->bin_n_small, out->n_unit[1] = c->bin_n_big;
	return 0;
}

// the roundings of a final arc record on the device (k_genes.hpp: arc_final_hi): out[4 n] = {avg_dist, s1, s2, 0} of every in[i]
extern "C" int pga_selftest_arc_final(const pga_arc_part_t *in, int64_t n, int32_t *out)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PGA_ERR_NO_DEVICE;
	if (n <= 0 || in == nullptr || out == nullptr) return PGA_ERR_ARG;
	pga_arc_part_t *di; int4 *dout;
	HIPCHK(hipMalloc((void **)&di, sizeof(pga_arc_part_t) * (size_t)n)); HIPCHK(hipMalloc((void **)&dout, sizeof(int4) * (size_t)n));
	HIPCHK(hipMemcpy(di, in, sizeof(pga_arc_part_t) * (size_t)n, hipMemcpyHostToDevice));
	hipLaunchKernelGGL(k_arc_final_probe, dim3(nblk(n)), dim3(BLOCK), 0, 0, (const pga_arc_part_t *)di, n, dout);
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(out, dout, sizeof(int4) * (size_t)n, hipMemcpyDeviceToHost));
	(void)hipFree(di); (void)hipFree(dout);
	return 0;
}

// k_post_count + k_post_rep (k_stage_b.hpp) on given protein sums, without a context (tests/test_front_gpu.py): sums[6 P] as pga_post_partials leaves them
// BEFORE k_post_count (plane 1 is overwritten), words[16 + 3 P + Q] / rep[P] / pj[P] as pga_post_front leaves them
extern "C" int pga_selftest_post_rep(const int64_t *sums, const int32_t *max_ori, const int32_t *prot_gid, int32_t P, int32_t Q, double min_cnt, int32_t joint_pseudo, int32_t drop_sgl_exon,
                                     int32_t *words, uint8_t *rep, uint8_t *pj)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PGA_ERR_NO_DEVICE;
	if (P <= 0 || Q <= 0 || !sums || !max_ori || !prot_gid || !words || !rep || !pj) return PGA_ERR_ARG;
	const size_t nw = 16 + 3 * (size_t)P + (size_t)Q;
	unsigned long long *d_sums, *d_key; int32_t *d_mx, *d_gid, *d_rep1, *d_words; uint8_t *d_rep;
	HIPCHK(hipMalloc((void **)&d_sums, sizeof(int64_t) * 6 * (size_t)P)); HIPCHK(hipMalloc((void **)&d_key, sizeof(int64_t) * (size_t)Q));
	HIPCHK(hipMalloc((void **)&d_mx, sizeof(int32_t) * (size_t)P)); HIPCHK(hipMalloc((void **)&d_gid, sizeof(int32_t) * (size_t)P));
	HIPCHK(hipMalloc((void **)&d_rep1, sizeof(int32_t) * (size_t)Q));
	HIPCHK(hipMalloc((void **)&d_words, sizeof(int32_t) * nw)); HIPCHK(hipMalloc((void **)&d_rep, 2 * (size_t)P));
	HIPCHK(hipMemcpy(d_sums, sums, sizeof(int64_t) * 6 * (size_t)P, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(d_mx, max_ori, sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(d_gid, prot_gid, sizeof(int32_t) * (size_t)P, hipMemcpyHostToDevice));
	HIPCHK(hipMemset(d_key, 0, sizeof(int64_t) * (size_t)Q)); HIPCHK(hipMemset(d_rep1, 0, sizeof(int32_t) * (size_t)Q));
	HIPCHK(hipMemset(d_words, 0, sizeof(int32_t) * 16)); HIPCHK(hipMemset(d_words + 16, 0xff, sizeof(int32_t) * (nw - 16)));
	hipLaunchKernelGGL(k_post_count, dim3(nblk(P)), dim3(BLOCK), 0, 0, d_sums, P, (const int32_t *)d_gid, Q, d_key);
	PostFront a = { d_sums, d_mx, d_gid, P, Q, min_cnt, joint_pseudo ? 1 : 0, drop_sgl_exon ? 1 : 0, d_key, d_rep1, d_rep, d_rep + P, d_words };
	hipLaunchKernelGGL(k_post_rep, dim3(nblk(P)), dim3(BLOCK), 0, 0, a);
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(words, d_words, sizeof(int32_t) * nw, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(rep, d_rep, (size_t)P, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(pj, d_rep + P, (size_t)P, hipMemcpyDeviceToHost));
	(void)hipFree(d_sums); (void)hipFree(d_key); (void)hipFree(d_mx); (void)hipFree(d_gid); (void)hipFree(d_rep1); (void)hipFree(d_words); (void)hipFree(d_rep);
	return 0;
}
