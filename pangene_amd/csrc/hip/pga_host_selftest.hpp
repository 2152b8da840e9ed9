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

// which builds of the sweep and of stage A's filters a context takes (tests/test_sweep_gpu.py, tests/support/sweep_direct.py): out[6] =
// {lists_in_lds, density_known, any_multi, exon_regular, gf_ok, gf_k32}.  Reads only; not part of pangene_hip.h.
extern "C" int pga_selftest_sweep_route(pga_ctx_t *c, int32_t *out)
{
	if (c == nullptr || out == nullptr) return PGA_ERR_ARG;
	out[0] = c->lists_in_lds, out[1] = c->density_known, out[2] = c->any_multi, out[3] = c->exon_regular, out[4] = c->gf_ok, out[5] = c->gf_k32;
	return 0;
}

// which route the arc and branch rounds of a context took (tests/test_arcs_gpu.py, tests/support/arcs_direct.py): out[8] = {n_big = ga_ctl[0] as the
// last arc round left it (the genes k_gene_arcs_wave_t handed on), the genes that overflowed their table in the last round as mailed, table_sparse,
// live_on, NL, rp_form, positions a thread of the walk that ran (1 or 4; 0: none), lds_vtx_set != 0}.  Waits for the stream; reads only; not part of
// pangene_hip.h.
extern "C" int pga_selftest_arc_route(pga_ctx_t *c, int32_t *out)
{
	if (c == nullptr || out == nullptr) return PGA_ERR_ARG;
	TRY(sync_st(c));
	int32_t n_big = 0;
	if (c->ga_ctl) HIPCHK(hipMemcpy(&n_big, c->ga_ctl, sizeof(int32_t), hipMemcpyDeviceToHost));
	// (a round of pga_arc_round_local leaves its own count behind the counters and degrees it mails, where later mail does not reach it: out[1] is valid
	// directly behind such a round only -- after pga_arc_round, a forced sort path or an exchange round the slot is stale or holds something else)
	out[0] = n_big, out[1] = c->h_round ? c->h_round[4 * (size_t)c->n_seg] : (int32_t)c->h_cnt[9], out[2] = c->table_sparse, out[3] = c->live_on, out[4] = c->NL, out[5] = c->rp_form, out[6] = c->walk_ipt, out[7] = c->lds_vtx_set != 0;
	return 0;
}

// what the order overrides keep current beside the arrays pga_selftest_stage_a exports (tests/test_order_gpu.py, tests/support/order_direct.py): inv, the
// gene-major index's zpos / zx, and under live lists lx, the members' list in cm order and their compact records; with the route of the context's last
// pga_override_order = {which, T, z_keep, wrec_ok, partial, live, h_ov grew, ov_seq}.  Waits for the stream; reads only; not part of pangene_hip.h.
typedef struct {
	int32_t *inv, *zpos, *zx;      /* [N] each (zx: the first NL entries mean something) */
	int32_t *lx;                   /* [N + 1] */
	int32_t *ylist;                /* [N]: the first NL entries of what the walk reads */
	int32_t *cA, *cB, *cC, *cx;    /* [4 N] [4 N] [4 N] [N]: the first NL entries */
	int32_t NL, live_on, z_valid, inv_valid, wrec_valid, ha_valid, zposy_stale; /* out */
	int32_t route[8];              /* out */
	uint32_t f_member;             /* out: the value of the internal bit "in the live lists" */
} pga_selftest_order_t;
extern "C" int pga_selftest_order(pga_ctx_t *c, pga_selftest_order_t *out) // any pointer may be NULL
{
	if (c == nullptr || out == nullptr) return PGA_ERR_ARG;
	TRY(sync_st(c));
	const size_t N = (size_t)c->N, NL = (size_t)c->NL;
	auto fetch = [&](void *dst, const void *src, size_t bytes) { return (dst == nullptr || src == nullptr || bytes == 0 || hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost) == hipSuccess) ? 0 : PGA_ERR_NO_DEVICE; };
	TRY(fetch(out->inv, c->inv, sizeof(int32_t) * N)); TRY(fetch(out->zpos, c->zpos, sizeof(int32_t) * N)); TRY(fetch(out->zx, c->zx, sizeof(int32_t) * N));
	if (N) TRY(fetch(out->lx, c->lx, sizeof(int32_t) * (N + 1)));
	TRY(fetch(out->ylist, c->ylist, sizeof(int32_t) * std::min(N, NL)));
	if (c->live_on) {
		TRY(fetch(out->cA, c->cA, sizeof(int4) * std::min(N, NL))); TRY(fetch(out->cB, c->cB, sizeof(int4) * std::min(N, NL))); TRY(fetch(out->cC, c->cC, sizeof(int4) * std::min(N, NL)));
		TRY(fetch(out->cx, c->cx, sizeof(int32_t) * std::min(N, NL)));
	}
	out->NL = c->NL, out->live_on = c->live_on, out->z_valid = c->z_valid, out->inv_valid = c->inv_valid, out->wrec_valid = c->wrec_valid, out->ha_valid = c->ha_valid, out->zposy_stale = c->zposy_stale;
	memcpy(out->route, c->ov_route, sizeof(out->route));
	out->f_member = F_MEMBER;
	return 0;
}

// What the last pga_branch_loop of the context did with PANGENE_LOOP_LEAN (read-only; ten words): out[0] the parts that were on (the bit mask; 0: every launch as
// before), [1] sweeps of that call that evaluated their open hits themselves, [2] how many open hits those evaluated, [3] k_gene_arcs_big was left out,
// [4] status-4 repeats for a gene that needed it, counted over the upload, [5] the longest slow list of a MODE-0 sweep since the upload as the host
// knows it (-1: not seen yet), [6] the upload keeps k_gene_arcs_big from now on, [7] sweeps of that call that applied the round's k_flag_vtx while staging (bit 8), [8] the segments that call ran over, [9] calls of pga_branch_loop in this process that got as far as their wait.
// c == NULL: the last such call of the process, whatever its context (a run through the pg_* entry points has no handle on the context).
extern "C" int pga_selftest_loop_route(pga_ctx_t *c, int32_t *out)
{
	if (out == nullptr) return PGA_ERR_ARG;
	std::lock_guard<std::mutex> lk(g_loop_route_mu);
	if (c) { // (with the context at hand: [1] and [2] count the sweeps since that call began as well -- pga_shadow with PANGENE_SWEEP_INLINE=1)
		TRY(sync_st(c));
		int64_t n_inline = 0;
		HIPCHK(hipMemcpy(&n_inline, c->dcnt + 20, sizeof(int64_t), hipMemcpyDeviceToHost));
		loop_route_of(c, out), out[2] = (int32_t)std::min<int64_t>(n_inline, INT32_MAX), out[9] = g_loop_route[9];
	}
	else memcpy(out, g_loop_route, sizeof(g_loop_route));
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

// pg_mark_branch_flt_arc's device chain on a given arc table and a given position-record table (tests/test_branch_lazy_gpu.py): counts -> offsets ->
// list -> k_n_local -> decision (-> residual list -> k_n_local -> k_br_finish when lazy), the kernels and host steps pga_branch_loop queues, without a
// context of a data set.  vs / ve [n_vtx]: the arc range of every vertex; s1 / agid [n_arc]: rounded score and target gene of every arc; rp [4 Q GL]:
// the full-form records {contig, rank, cm, interval} of (gene, genome), contig -1 = absent.  lazy: 0 every pair, 1 the lazy form; res_cap: room of
// the residual list on the first attempt (<= 0: the floor; shared out over BR_RSEG segments) -- a list beyond it ends in the repeat with room, as pga_branch_loop's status 4 does;
// gate_closed: every launch finds its gate closed (the outputs stay as the caller filled them).  aw [n_arc], ndl [n_vtx], vwk [n_vtx]: in / out;
// lens[4]: the main list's length, the residual list's, attempts made, the sticky flag of the LAST attempt.
extern "C" int pga_selftest_branch(const int32_t *vs, const int32_t *ve, const int32_t *s1, const int32_t *agid, int32_t n_vtx, int64_t n_arc, const int32_t *rp, int32_t Q, int32_t GL,
                                   double bd, double bdist, double bcut, int32_t local_dist, int32_t local_count, int32_t lazy, int64_t res_cap, int32_t gate_closed,
                                   uint8_t *aw, int32_t *ndl, uint8_t *vwk, int64_t *lens)
{
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return PGA_ERR_NO_DEVICE;
	if (n_vtx <= 0 || n_vtx > PO_THREADS * PO_MAX_ITEMS || n_arc <= 0 || Q <= 0 || GL <= 0 || !vs || !ve || !s1 || !agid || !rp || !aw || !ndl || !vwk || !lens) return PGA_ERR_ARG;
	for (int v = 0; v < n_vtx; ++v) if (vs[v] < 0 || ve[v] < vs[v] || ve[v] > n_arc) return PGA_ERR_ARG;
	for (int64_t i = 0; i < n_arc; ++i) if (agid[i] < 0 || agid[i] >= Q || s1[i] <= 0) return PGA_ERR_ARG;
	pga_ctx c; // a bare context: stream, counters, pool
	HIPCHK(hipStreamCreateWithFlags(&c.st, hipStreamNonBlocking));
	TRY(dalloc(&c, &c.dcnt, 24)); TRY(dalloc(&c, &c.loopctl, 4)); TRY(dalloc_commit(&c));
	HIPCHK(hipHostMalloc((void **)&c.h_cnt, 24 * sizeof(int64_t), hipHostMallocDefault));
	HIPCHK(hipHostGetDevicePointer((void **)&c.h_box, c.h_cnt, 0));
	c.n_genome = GL, c.Q = Q, c.rp_form = RP_FULL;
	c.br_n = n_arc, c.br_S = n_vtx / 2, c.br_np = -1;
	c.br_par.diff = bd, c.br_par.local_dist = local_dist, c.br_par.local_count = local_count, c.br_par.frag_mode = 0;
	auto up = [&](int slot, const void *src, size_t bytes) -> void * { void *d = c.pool.get(slot, bytes + 16); if (d && hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, c.st) != hipSuccess) d = nullptr; return d; };
	int32_t *d_vs = (int32_t *)up(S_BR_VS, vs, sizeof(int32_t) * (size_t)n_vtx), *d_ve = (int32_t *)up(S_BR_VE, ve, sizeof(int32_t) * (size_t)n_vtx);
	int32_t *d_s1 = (int32_t *)up(S_BR_S1, s1, sizeof(int32_t) * (size_t)n_arc), *d_gid = (int32_t *)up(S_BR_GID, agid, sizeof(int32_t) * (size_t)n_arc);
	void *d_rp = up(S_RP_SEG, rp, sizeof(int4) * (size_t)Q * (size_t)GL);
	uint8_t *d_aw = (uint8_t *)up(S_ARCW, aw, (size_t)n_arc), *d_vwk = (uint8_t *)up(S_VWK, vwk, (size_t)n_vtx);
	int32_t *d_ndl = (int32_t *)up(S_BR_NDL, ndl, sizeof(int32_t) * (size_t)n_vtx);
	int32_t *pc = (int32_t *)c.pool.get(S_BR_PC, sizeof(int32_t) * (loop_btot_at(n_vtx) + 64) + 16), *poff = (int32_t *)c.pool.get(S_BR_POFF, sizeof(int32_t) * (size_t)n_vtx + 16);
	int32_t *grp = (int32_t *)c.pool.get(S_BR_GRP, sizeof(int32_t) * (size_t)n_arc + 16);
	int rc = (d_vs && d_ve && d_s1 && d_gid && d_rp && d_aw && d_vwk && d_ndl && pc && poff && grp && c.pool.get(S_RP_IV, 16)) ? 0 : PGA_ERR_NOMEM;
	if (rc == 0 && (hipMemsetAsync(c.dcnt, 0, 24 * sizeof(int64_t), c.st) != hipSuccess || hipMemsetAsync(c.loopctl, 0xff, 4 * sizeof(int32_t), c.st) != hipSuccess)) rc = PGA_ERR_NO_DEVICE;
	// the worst case of the main list, so that only the residual list can run out of room: n^2 pairs a vertex (branch.c:70-88)
	int64_t worst = 16;
	for (int v = 0; v < n_vtx; ++v) worst += (int64_t)(ve[v] - vs[v]) * (ve[v] - vs[v]);
	c.br_cap = worst;
	c.gate = gate_closed ? Gate{c.loopctl, 0} : Gate{nullptr, 0}; // (loopctl = {-1, -1, ..}: nothing has happened in round 0 or later)
	c.br_lazy = lazy != 0;
	c.br_rcap = res_cap > 0 ? res_cap : (int64_t)1 << 16;
	if (rc == 0 && c.br_lazy && (!br_res_len(&c) || hipMemsetAsync(br_res_len(&c), 0, sizeof(int64_t) * BR_RSEG * BR_RSTRIDE, c.st) != hipSuccess)) rc = PGA_ERR_NOMEM; // (a closed gate starts nothing)
	int attempt = 0;
	for (; rc == 0; ++attempt) {
		BrLazy lz;
		if ((rc = br_lazy_args(&c, n_vtx, &lz)) != 0) break;
		(void)hipMemsetAsync(c.dcnt + 11, 0, sizeof(int64_t), c.st);
		(void)hipMemsetAsync(c.dcnt + 15, 0, 4 * sizeof(int64_t), c.st);
		hipLaunchKernelGGL(k_br_count, dim3(nblk(n_vtx)), dim3(BLOCK), 0, c.st, n_vtx, (const int32_t *)d_vs, (const int32_t *)d_ve, (const int32_t *)d_s1, bd, pc, c.gate, br_res_len(&c));
		hipLaunchKernelGGL(k_pair_offsets, dim3(1), dim3(PO_THREADS), 0, c.st, (const int32_t *)pc, n_vtx, poff, c.dcnt, c.h_box, (long long)c.br_cap, c.gate);
		int32_t *cnt;
		if ((rc = branch_enumerate(&c, &cnt)) != 0) break;
		hipLaunchKernelGGL((k_br_wave<2>), dim3(nblk(n_vtx, BLOCK / WAVE)), dim3(BLOCK), 0, c.st, n_vtx, (const int32_t *)d_vs, (const int32_t *)d_ve, (const int32_t *)d_s1, (const int32_t *)d_gid, bd, (const int32_t *)poff, (int32_t *)nullptr, (int64_t)c.br_cap,
		                   (const int32_t *)nullptr, (const int32_t *)cnt, bdist, bcut, d_aw, grp, d_ndl, (int64_t *)nullptr, d_vwk, (const int64_t *)(c.dcnt + 15), c.gate, lz);
		if ((rc = branch_residual(&c, lz, n_vtx, d_ndl)) != 0) break;
		if (hipMemcpyAsync(c.h_cnt, c.dcnt, 24 * sizeof(int64_t), hipMemcpyDeviceToHost, c.st) != hipSuccess || hipStreamSynchronize(c.st) != hipSuccess) { rc = PGA_ERR_NO_DEVICE; break; }
		if (c.h_cnt[11] && c.br_lazy && c.h_cnt[18] * BR_RSEG > c.br_rcap && attempt == 0) { // the residual list did not fit: the repeat with room (the arcs' marks start again, as the caller's next run does)
			c.br_rcap = c.h_cnt[18] * BR_RSEG + c.h_cnt[18] * BR_RSEG / 4;
			(void)hipMemcpyAsync(d_aw, aw, (size_t)n_arc, hipMemcpyHostToDevice, c.st); (void)hipMemcpyAsync(d_vwk, vwk, (size_t)n_vtx, hipMemcpyHostToDevice, c.st);
			(void)hipMemcpyAsync(d_ndl, ndl, sizeof(int32_t) * (size_t)n_vtx, hipMemcpyHostToDevice, c.st);
			continue;
		}
		++attempt;
		break;
	}
	if (rc == 0) {
		lens[0] = c.h_cnt[15], lens[1] = 0, lens[2] = attempt, lens[3] = c.h_cnt[11];
		int64_t seg_len[BR_RSEG] = { 0 };
		if (c.br_lazy && hipMemcpy2D(seg_len, sizeof(int64_t), br_res_len(&c), sizeof(int64_t) * BR_RSTRIDE, sizeof(int64_t), BR_RSEG, hipMemcpyDeviceToHost) != hipSuccess) rc = PGA_ERR_NO_DEVICE;
		for (int k = 0; k < BR_RSEG; ++k) lens[1] += seg_len[k];
		if (hipMemcpy(aw, d_aw, (size_t)n_arc, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(vwk, d_vwk, (size_t)n_vtx, hipMemcpyDeviceToHost) != hipSuccess ||
		    hipMemcpy(ndl, d_ndl, sizeof(int32_t) * (size_t)n_vtx, hipMemcpyDeviceToHost) != hipSuccess) rc = PGA_ERR_NO_DEVICE;
	}
	(void)hipStreamSynchronize(c.st);
	(void)hipHostFree(c.h_cnt); c.h_cnt = nullptr, c.h_box = nullptr;
	c.pool.release();
	for (void *q : c.owned) (void)hipFree(q);
	dev_big_free(c.arena, c.arena_cap), c.arena = nullptr;
	(void)hipStreamDestroy(c.st); c.st = nullptr;
	return rc;
}
