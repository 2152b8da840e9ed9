// pga_host_stage_b.hpp -- pg_post_process (graph.c:7-32) and the vertex partials (vertex.c:28-51).
// Host side of the device ABI (include/pangene_hip.h); included by pga_backend.hip (one translation unit), in this order.
#pragma once


// the tables of pga_post_front: per gene the largest key of its proteins and the representative (+ 1); per protein the two bytes k_post_apply reads
struct FrontTabs { unsigned long long *gene_key; int32_t *gene_rep1; uint8_t *rep, *pj; };
static bool front_tabs(pga_ctx *c, FrontTabs *t)
{
	const size_t Q = (size_t)std::max(1, c->Q), P = (size_t)std::max(1, c->P);
	char *b = (char *)c->pool.get(S_FRONT, 12 * Q + 2 * P + 64);
	if (!b) return false;
	t->gene_key = (unsigned long long *)b, t->gene_rep1 = (int32_t *)(b + 8 * Q), t->rep = (uint8_t *)(b + 12 * Q), t->pj = t->rep + P;
	return true;
}

extern "C" int pga_post_partials(pga_ctx_t *c, int32_t **max_ori, int64_t **sums)
{
	FrontTabs ft;
	if (!front_tabs(c, &ft)) return PGA_ERR_NOMEM;
	// The genes' largest keys (what pga_post_front picks the representatives by) ride with this call's clear and with k_post_count -- where a post_front is to be
	// expected: a context whose last pg_post_process went on with post_apply instead (a sharded run, PANGENE_FRONT=host, a data set with tied isoforms, a verbose
	// log) leaves them out, and a post_front that comes all the same makes up for it (front_keys)
	const bool keys = c->front_keys_on;
	c->front_keys_done = keys;
	zero_multi(c, c->max_ori, sizeof(int32_t) * (size_t)std::max(1, c->P), c->sums, sizeof(int64_t) * 6 * (size_t)std::max(1, c->P),
	           keys ? ft.gene_key : nullptr, keys ? 12 * (size_t)std::max(1, c->Q) : 0); // (gene_key and gene_rep1 lie side by side)
	// (round 6) the sums through LDS where the proteins fit in one or two ranges and a workgroup's stretch is long enough to hold several genomes
	static const bool pp_atomics = env_has("PANGENE_POST", "atomics"); // (tests: the one-atomic-a-contribution form on every shard)
	static const bool pp_force = env_has("PANGENE_POST", "lds");       // (tests: the LDS form on small shards too)
	bool lds_done = false;
	if (c->N && c->P && !pp_atomics && (c->N >= (1 << 19) || pp_force)) {
		const size_t room = (size_t)144 << 10;
		const int p_tiles = (size_t)c->P * 28 <= room ? 1 : (size_t)((c->P + 1) / 2) * 28 <= room ? 2 : 0;
		if (p_tiles) {
			const int PT = (c->P + p_tiles - 1) / p_tiles;
			const size_t lds = (size_t)PT * 28 + 16;
			bool ok = true; // (the attribute belongs to the device the context runs on: kept per context, and a launch that is refused leaves the step to k_post_part)
			if (lds > c->lds_post_set) { ok = hipFuncSetAttribute(reinterpret_cast<const void *>(k_post_part_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess; if (ok) c->lds_post_set = lds; else (void)hipGetLastError(); }
			if (ok) {
				const int n_chunk = (int)std::max<int64_t>(1, std::min<int64_t>(c->n_cu, c->N / 32768)); // (a stretch of >= 32 k hits: the reduction is what the launch is for)
				(void)hipGetLastError(); // (what is read below is this launch's)
				hipLaunchKernelGGL(k_post_part_lds, dim3((unsigned)(n_chunk * p_tiles)), dim3(PP_T), lds, c->st, c->flags, c->pid, c->rank, c->sori, c->sadj, c->nex, c->N, c->P, p_tiles, PT,
				                   c->max_ori, (unsigned long long *)c->sums);
				lds_done = hipGetLastError() == hipSuccess;
				if (!lds_done) c->lds_post_set = 0;
			}
		}
	}
	if (c->N && !lds_done) hipLaunchKernelGGL(k_post_part, dim3(nblk(c->N)), dim3(BLOCK), 0, c->st, c->flags, c->pid, c->rank, c->sori, c->sadj, c->nex, c->N, c->P,
	                             c->max_ori, (unsigned long long *)c->sums);
	if (c->N && c->P) hipLaunchKernelGGL(k_post_count, dim3(nblk(c->P)), dim3(BLOCK), 0, c->st, (unsigned long long *)c->sums, c->P, (const int32_t *)c->prot_gid, c->Q, keys ? ft.gene_key : (unsigned long long *)nullptr);
	*max_ori = c->max_ori, *sums = c->sums;
	return 0; // no wait: a consumer that is not on this stream calls pga_sync first
}

extern "C" int pga_post_apply(pga_ctx_t *c, const uint8_t *prot_rep, const uint8_t *prot_pj, int64_t *n_pseudo)
{
	c->yrec_valid = false, c->wrec_valid = false;
	c->front_keys_on = false; // (the caller picked the representatives itself: the next pga_post_partials need not prepare for a post_front)
	uint8_t *d = (uint8_t *)c->pool.get(S_MISC, 2 * (size_t)c->P + 16);
	if (!d) return PGA_ERR_NOMEM;
	c->walk_valid = false, c->ha_valid = false;
	TRY(stage_upload(c, d, prot_rep, (size_t)c->P, d + c->P, prot_pj, (size_t)c->P)); // caller memory
	if (n_pseudo) HIPCHK(hipMemsetAsync(c->dcnt + 2, 0, sizeof(int64_t), c->st));
	if (c->N) hipLaunchKernelGGL(k_post_apply, dim3(nblk(c->N)), dim3(BLOCK), 0, c->st, c->flags, c->pid, c->nex, c->sdom, c->N, c->max_ori, d, d + c->P, n_pseudo ? c->dcnt + 2 : (int64_t *)nullptr);
	if (n_pseudo) { // the count only feeds a log line: nobody waits for it otherwise
		HIPCHK(hipMemcpyAsync(c->h_cnt, c->dcnt, 16 * sizeof(int64_t), hipMemcpyDeviceToHost, c->st));
		TRY(sync_st(c));
		*n_pseudo = c->h_cnt[2];
	}
	return 0;
}

// pga_post_apply without the host in front of it (include/pangene_hip.h): behind pga_post_partials on the same stream, nothing in between that touches the sums
extern "C" int pga_post_front(pga_ctx_t *c, double min_cnt, int32_t joint_pseudo, int32_t drop_sgl_exon, const int32_t **host_view)
{
	FrontTabs ft;
	if (host_view == nullptr) return PGA_ERR_ARG;
	if (!front_tabs(c, &ft)) return PGA_ERR_NOMEM;
	const size_t P = (size_t)c->P, Q = (size_t)c->Q, words = 16 + 3 * P + Q;
	if (c->front_live && c->front_epoch == c->sync_epoch) TRY(sync_st(c)); // nobody has waited since the last one was queued: the area is still the device's
	if (c->h_front_cap < words) {
		c->h_front = (int32_t *)c->pin.get(sizeof(int32_t) * (words + words / 2) + 256); // (the old piece stays in the arena)
		if (!c->h_front) { c->h_front_cap = 0; return PGA_ERR_NOMEM; }
		c->h_front_cap = words + words / 2;
	}
	memset(c->h_front, 0, sizeof(int32_t) * 16);
	if (Q) memset(c->h_front + 16 + 3 * P, 0xff, sizeof(int32_t) * Q); // rep_pid = -1
	int32_t *hd = nullptr;
	HIPCHK(hipHostGetDevicePointer((void **)&hd, c->h_front, 0));
	c->yrec_valid = false, c->wrec_valid = false, c->walk_valid = false, c->ha_valid = false; // (as pga_post_apply)
	if (!c->front_keys_done) { // pga_post_partials did not expect this call: the genes' keys now (k_post_count once more -- it writes the counts it wrote before)
		zero_multi(c, ft.gene_key, 12 * (size_t)std::max(1, c->Q));
		if (c->N && c->P) hipLaunchKernelGGL(k_post_count, dim3(nblk(c->P)), dim3(BLOCK), 0, c->st, (unsigned long long *)c->sums, c->P, (const int32_t *)c->prot_gid, c->Q, ft.gene_key);
		c->front_keys_done = true;
	}
	c->front_keys_on = true;
	PostFront a = { (const unsigned long long *)c->sums, c->max_ori, c->prot_gid, c->P, c->Q, min_cnt, joint_pseudo ? 1 : 0, drop_sgl_exon ? 1 : 0, ft.gene_key, ft.gene_rep1, ft.rep, ft.pj, hd };
	if (c->P) hipLaunchKernelGGL(k_post_rep, dim3(nblk(c->P)), dim3(BLOCK), 0, c->st, a);
	if (c->N) hipLaunchKernelGGL(k_post_apply, dim3(nblk(c->N)), dim3(BLOCK), 0, c->st, c->flags, c->pid, c->nex, c->sdom, c->N, c->max_ori, (const uint8_t *)ft.rep, (const uint8_t *)ft.pj, (int64_t *)nullptr);
	c->front_live = true, c->front_epoch = c->sync_epoch;
	*host_view = c->h_front;
	return 0; // no wait: the view holds what it promises after the caller's next wait for the stream
}

extern "C" int pga_shadow(pga_ctx_t *c, int32_t cal_dom_sc, int32_t *stats)
{
	c->yrec_valid = false, c->wrec_valid = false;
	if (cal_dom_sc) TRY(launch_sweep<1>(c, -1)); else TRY(launch_sweep<0>(c, 2));
	if (stats) {
		int32_t *d_stats = (int32_t *)c->pool.get(S_STATS, sizeof(int32_t) * 4 * (size_t)c->n_genome + 16);
		if (!d_stats) return PGA_ERR_NOMEM;
		HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(int32_t) * 2 * (size_t)c->n_genome + 16, c->st));
		if (c->N) hipLaunchKernelGGL(k_count_shadow, dim3(nblk(c->N)), dim3(BLOCK), 0, c->st, c->flags, c->gnm, c->N, d_stats);
		HIPCHK(hipMemcpyAsync(stats, d_stats, sizeof(int32_t) * 2 * (size_t)c->n_genome, hipMemcpyDeviceToHost, c->st));
		return sync_st(c);
	}
	return 0;
}

extern "C" int pga_set_filter(pga_ctx_t *c, int32_t which)
{
	if (which < 0 || which > 3) return PGA_ERR_ARG;
	const bool queued = c->shadow_queued; // (pga_branch_loop with final_on queued this very filter behind its last arc round, and nothing has touched the hits since)
	c->shadow_queued = false;
	if (queued && which == PGA_FLT_SHADOW) return 0;
	c->walk_valid = false, c->ha_valid = false;
	if (c->N) hipLaunchKernelGGL(k_set_filter, dim3(nblk(c->N)), dim3(BLOCK), 0, c->st, c->flags, c->N, which);
	return 0;
}

static int check_invariant(pga_ctx *c, bool flushed = false) // flushed: a k_mail_sum just sent the counters to the host mirror
{
	if (!flushed) hipLaunchKernelGGL(k_mail_flush, dim3(1), dim3(64), 0, c->st, c->dcnt, c->h_box);
	TRY(sync_st(c));
	return c->h_cnt[3] ? PGA_ERR_INVARIANT : 0;
}

extern "C" int pga_vtx_partials(pga_ctx_t *c, int32_t **cnt, uint64_t **records, int64_t *n_records)
{
	const int N = c->N, Q = c->Q, GL = c->n_genome;
	const int64_t wpg = (Q + 31) / 32, n_slot = (int64_t)std::max(1, Q) * VTX_K;
	const int nw = (c->n_genome_global + 63) / 64;
	static const long long first_cap = [] { const char *e = getenv("PANGENE_VTX_SPILL_CAP"); return e && atoll(e) > 0 ? atoll(e) : 65536ll; }(); // (tests shrink it to reach the second attempt)
	long long ovf_cap = first_cap;
	uint32_t *bits = (uint32_t *)c->pool.get(S_BITS, sizeof(uint32_t) * (size_t)(wpg * GL) + 16);
	if (!bits) return PGA_ERR_NOMEM;
	*n_records = 0, *cnt = c->vtx_cnt;
	for (int attempt = 0;; ++attempt) { // the spill area beyond the VTX_K dominator slots per gene grows to what the first attempt counted
		// [dom_tab: n_slot i32][slot: n_slot i32][pair bits: n_slot * nw u64][records: (n_slot + ovf_cap) * (1 + nw) u64]
		const size_t b_tab = sizeof(int32_t) * (size_t)n_slot, b_bits = sizeof(uint64_t) * (size_t)n_slot * (size_t)nw, b_rec = sizeof(uint64_t) * (size_t)(n_slot + ovf_cap) * (size_t)(1 + nw);
		char *blk = (char *)c->pool.get(S_TRIPLES, 2 * b_tab + b_bits + b_rec + 64);
		if (!blk) return PGA_ERR_NOMEM;
		int32_t *dom_tab = (int32_t *)blk, *slot = (int32_t *)(blk + b_tab);
		unsigned long long *pbits = (unsigned long long *)(blk + 2 * b_tab), *rec = (unsigned long long *)(blk + 2 * b_tab + b_bits);
		zero_multi(c, bits, sizeof(uint32_t) * (size_t)(wpg * GL) + 16, c->vtx_cnt, sizeof(int32_t) * 2 * (size_t)std::max(1, Q), c->dcnt, sizeof(int64_t), pbits, b_bits);
		HIPCHK(hipMemsetAsync(dom_tab, 0xff, b_tab, c->st)); // every slot empty (-1)
		HIPCHK(hipMemsetAsync(c->live_cnt, 0, sizeof(int64_t) * LIVE_CNT_N, c->st)); // k_vtx1 counts the hits without flt there
		*records = (uint64_t *)rec;
		if (N == 0) return sync_st(c);
		{ // (round 6) the genes' counts through LDS on shards whose stretches hold several genomes (PANGENE_POST=atomics / lds as for k_post_part_lds)
			static const bool vx_atomics = env_has("PANGENE_POST", "atomics"), vx_force = env_has("PANGENE_POST", "lds");
			const size_t lds = sizeof(int) * 2 * (size_t)std::max(1, Q);
			bool ok = !vx_atomics && (N >= (1 << 19) || vx_force) && lds <= ((size_t)144 << 10); // (the attribute per context and the launch checked, as in pga_post_partials)
			if (ok && lds > c->lds_vtx_set) { ok = hipFuncSetAttribute(reinterpret_cast<const void *>(k_vtx1_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess; if (ok) c->lds_vtx_set = lds; else (void)hipGetLastError(); }
			if (ok) {
				const int n_chunk = (int)std::max<int64_t>(1, std::min<int64_t>(2 * c->n_cu, N / 32768));
				(void)hipGetLastError(); // (what is read below is this launch's)
				hipLaunchKernelGGL(k_vtx1_lds, dim3((unsigned)n_chunk), dim3(VX_T), lds, c->st, c->flags, c->gnm, c->gid, c->rank, c->pdom, N, Q, c->vtx_cnt, bits, wpg, c->dcnt, c->live_cnt);
				ok = hipGetLastError() == hipSuccess;
				if (!ok) c->lds_vtx_set = 0;
			}
			if (!ok)
			hipLaunchKernelGGL(k_vtx1, dim3(nblk(N)), dim3(BLOCK), 0, c->st, c->flags, c->gnm, c->gid, c->rank, c->pdom, N, Q, c->vtx_cnt, bits, wpg, c->dcnt, c->live_cnt);
		}
		hipLaunchKernelGGL(k_live_sum, dim3(1), dim3(BLOCK), 0, c->st, (const int64_t *)c->live_cnt, c->dcnt);
		hipLaunchKernelGGL(k_vtx_fold, dim3(nblk(N)), dim3(BLOCK), 0, c->st, c->flags, c->gnm, c->gid, c->rank, c->pdom, c->prot_gid, c->ggl, N, bits, wpg,
		                   dom_tab, pbits, nw, rec + n_slot * (1 + nw), ovf_cap, c->dcnt);
		I32 *tile = (I32 *)c->pool.get(S_TILE, tile_buf_bytes(n_slot));
		if (!tile) return PGA_ERR_NOMEM;
		device_scan<I32>(InDomSet{dom_tab}, OutExclI32{slot}, n_slot, tile, OpSum{}, I32{0}, c->st);
		hipLaunchKernelGGL(k_vtx_compact, dim3(nblk(n_slot)), dim3(BLOCK), 0, c->st, dom_tab, slot, n_slot, pbits, nw, rec, c->dcnt, c->h_box);
		// Behind a pga_post_front that nobody has waited for since, this is the first wait since stage A was queued: 0.7 ms at configs[1] where the two waits it replaces
		// took 0.4 each, so it polls for up to 1 ms before it parks.  (Some bench processes spend 0.35 ms a pass longer in the vertex step on the device route, for a
		// reason that is not known; with the longer poll it was 2 of 8 processes, without it 4 of 8 in the same session, 9 of 21 over two: DESIGN section 9, "slow mode".)
		const bool behind_front = c->front_live && c->front_epoch == c->sync_epoch;
		TRY(sync_st(c, behind_front ? 1000.0 : 200.0));
		if (c->h_cnt[3]) return PGA_ERR_INVARIANT;
		c->live_hint = c->h_cnt[8];
		const int64_t n_rec = c->h_cnt[10], n_ovf = c->h_cnt[0];
		if (n_ovf > ovf_cap) { // more spilled (genome, gene) cells than there was room for: once more, with room (the reference has no such limit)
			// which dominators win a gene's slots is a race, so the number of spilled cells may differ a little between attempts:
			// the second attempt gets a margin, a third one the upper bound (a spilled cell is at least one hit)
			if (ovf_cap >= (long long)N) return PGA_ERR_RANGE;
			ovf_cap = attempt == 0 ? std::min<long long>(N, 2 * n_ovf + 64) : (long long)N;
			continue;
		}
		if (n_ovf) { // the spilled single-genome records follow the folded ones
			HIPCHK(hipMemcpyAsync(rec + n_rec * (1 + nw), rec + n_slot * (1 + nw), sizeof(uint64_t) * (size_t)n_ovf * (size_t)(1 + nw), hipMemcpyDeviceToDevice, c->st));
			TRY(sync_st(c));
		}
		*n_records = n_rec + n_ovf;
		c->z_early = !c->z_valid; // (the caller fetches the records next and then computes for a while: pga_fetch)
		return 0;
	}
}

// Upload out of CALLER memory without waiting for it: the bytes (up to three pieces) are copied into a pinned staging area first,
// so the caller's buffers are free when the call returns and the DMA runs in stream order.
static int stage_upload(pga_ctx *c, void *d0, const void *s0, size_t n0, void *d1, const void *s1, size_t n1)
{
	const size_t a0 = (n0 + 15) & ~(size_t)15, nb = a0 + n1;
	if (nb == 0) return 0;
	if (c->h_g2s_cap < nb) {
		if (c->h_g2s) HIPCHK(hipStreamSynchronize(c->st)); // (the old piece stays in the arena)
		c->h_g2s = (int32_t *)c->pin.get(nb + nb / 2 + 64);
		if (!c->h_g2s) return PGA_ERR_NOMEM;
		c->h_g2s_cap = nb + nb / 2;
	}
	if (!c->g2s_done) HIPCHK(hipEventCreateWithFlags(&c->g2s_done, hipEventDisableTiming));
	else HIPCHK(hipEventSynchronize(c->g2s_done)); // the previous upload out of the staging area (long finished in practice)
	char *h = (char *)c->h_g2s;
	if (n0) memcpy(h, s0, n0);
	if (n1) memcpy(h + a0, s1, n1);
	if (nb <= ((size_t)1 << 20)) { // small: a copy kernel reads the staging area itself (see k_copy_in)
		char *hd = nullptr;
		HIPCHK(hipHostGetDevicePointer((void **)&hd, h, 0));
		CopyIn l = { { d0, d1 }, { (const uint32_t *)hd, (const uint32_t *)(hd + a0) }, { n0, n1 } };
		hipLaunchKernelGGL(k_copy_in, dim3(nblk((std::max(n0, n1) + 3) / 4)), dim3(BLOCK), 0, c->st, l);
	} else {
		if (n0) HIPCHK(hipMemcpyAsync(d0, h, n0, hipMemcpyHostToDevice, c->st));
		if (n1) HIPCHK(hipMemcpyAsync(d1, h + a0, n1, hipMemcpyHostToDevice, c->st));
	}
	HIPCHK(hipEventRecord(c->g2s_done, c->st));
	return 0;
}
