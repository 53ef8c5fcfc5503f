// primary_packet_body.h — the body of k_primary_packet and of k_primary_packet_masked (kernels.hip), included by both like
// shade_pt_body.h by the shade kernels: p, count, COUNT, ORDERED (the node table is camera-ordered: trace_packet); MASKED and `mask` (adaptive.h: one byte per slot tile) — with MASKED = false
// the kernel is the code it was before the masked one existed.  A group of a retired tile leaves void hit records and traces nothing.
// The ORDERED kernels, masked or not, start a group's walk from its record of the entry snapshot (primary_entry.h) where the launch
// carries the table (p.wv.primary_entry; null: the root); the sorting kernels and the counting ones (COUNT: the per-ray counters
// keep the meaning of a walk from the root) always start at the root.
	clock_in(p.wv.counters, 0);
	uint32_t *const head = &p.wv.counters->work[p.queue][0];
	const uint32_t lane = __lane_id();
	uint32_t run = count / (gridDim.x * (blockDim.x / 64u) * 4u);
	run = run > (uint32_t)RT_PACKET_CHUNK ? (uint32_t)RT_PACKET_CHUNK : (run < 64u ? 64u : (run & ~63u));
	TStat st;
	st.inner = 0, st.tris = 0, st.lds = 0;
	uint32_t nrays = 0;
	for (;;)
	{
		uint32_t g = 0;
		if (lane == 0)
			g = atomicAdd(head, run);
		g = (uint32_t)__builtin_amdgcn_readfirstlane((int)g);
		if (g >= count)
			break;
		const uint32_t end = g + run < count ? g + run : count;
		for (uint32_t base = g; base < end; base += 64u)
		{
			const uint32_t idx = base + lane;
			bool active = idx < end;
			if (MASKED)
			{
				// (base is wave-uniform: one scalar load of the word that holds the tile's byte)
				const Params &q = fresh_params();
				const uint32_t t = (uint32_t)__builtin_amdgcn_readfirstlane((int)ad_slot_tile(q.fr, base));
				if (((sload1u(mask, t & ~3u) >> ((t & 3u) * 8u)) & 0xffu) == 0u)
				{
					if (active)
						q.wv.hit0[idx] = ad_void_hit();
					unsigned char *const done = q.wv.hit0_done;
					if (done && lane == 0u)
						done[base >> 6] = 1;
					continue;
				}
			}
			f3 O = mk3(0, 0, 0), D = mk3(0, 0, 1);
			{
				const Params &q = fresh_params();
				if (active)
				{
					const PixelRef pr = slot_to_pixel(q.fr, idx);
					active = pr.valid;
					if (active)
						pt_primary_ray(q.cam, q.fr, pr.x, pr.y, q.fr.sample_base + pr.sample, O, D);
				}
			}
			Hit h;
			h.t = 1e34f, h.u = 0.0f, h.v = 0.0f, h.prim = -1, h.inst = -1;
			const uint32_t *entry = nullptr;
			if (ORDERED && !COUNT)
			{
				// (base is wave-uniform: scalar arithmetic) the group within its sample group: (slot mod (g * slots)) / 64
				const Params &q = fresh_params();
				const uint32_t *const table = q.wv.primary_entry;
				if (table)
					entry = table + (size_t)((base - fast_div(base, q.fr.div_group) * (q.fr.slots << q.fr.sgroup_log2)) >> 6) * PRIMARY_ENTRY_K;
			}
			trace_packet<COUNT, false, ORDERED>(fresh_params().sc, active, O, D, 1e-5f, h, st, entry);
			if (active)
			{
				primary_finish_item(fresh_params(), idx, D, h); // (hit record, or the sky term of a miss)
				nrays++;
			}
			// a group without a hit is finished here (27 % of the terrain's): the shade kernel's scan passes it by
			{
				unsigned char *const done = fresh_params().wv.hit0_done;
				const bool none = __ballot(active && h.prim >= 0) == 0ull;
				if (done && lane == 0u)
					done[base >> 6] = none ? 1 : 0;
			}
		}
	}
	if (COUNT)
	{
		WaveCounters *const wc = p.wv.counters;
		Ctx ctx;
		ctx.add64(&wc->inner_extend, st.inner);
		ctx.add64(&wc->tris_extend, st.tris);
		ctx.add64(&wc->rays_extend, nrays);
	}
	clock_out(p.wv.counters, 0);
