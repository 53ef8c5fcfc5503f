// adaptive.h — the work items of adaptive sampling (setting "adaptive_sampling", include/rfwhip.h): samples go only
// where the noise estimate (noise.h) says they are needed.  Included by kernels.hip inside namespace rtk, behind resolve_noise_item and
// present_item: the device kernels (k_extend_masked, k_primary_packet_masked, k_resolve_adaptive, k_present_adaptive,
// k_noise_tiles_adaptive, k_adaptive_step) and the host emulation (kernels_emu.inc) run the same items.  Nothing here is reached while
// the setting is off, and no kernel of the default path includes a line of it.
//
// UNIT: the noise tile, 32 x 8 pixels (NZ_TILE_*), aligned to the ownership strips: a tile belongs to one rank.  Per tile of a rank:
//   n_tile (uint32)   samples its pixels hold            active (byte)   1 until the tile retires
//   RESET / rfwhip_init: n_tile = 0, active = 1.  A retired tile stays retired until then, whatever the thresholds do later.
// MASK: what the primary wave reads — one byte per 8 x 8 SLOT tile (rt_core.h, slot_to_pixel; index ty * FrameView::tiles_x + tx), four
//   per noise tile (fewer at the right edge), 1 = trace.  A wave's 64 consecutive slots lie in one slot tile (a group of one tile is
//   64 g consecutive slots), so the lookup is wave-uniform.  A retired group traces nothing, its hit records say HIT_VOID — what the
//   shade kernels' scan already passes by — and, where the launch keeps group flags, its hit0_done byte says 1.
// A CALL of S samples per pixel: primary paths for the pixels of active tiles only, sample indices as ever (a retired pixel does not
//   draw its indices); k_resolve_adaptive = resolve_noise_item behind an early return, with n_a = n_tile (the slots of a retired
//   tile's pixels are never read); then k_adaptive_step: n_tile += S where active, and after every adaptive_every-th call since the
//   RESET the tile records of the metric at n = n_tile (k_noise_tiles_adaptive) decide:
//     an active tile retires when n_tile >= adaptive_min_samples and converged == pixels (every real pixel has e <= noise_threshold).
//   The mask call k + 1 reads is a function of the state after call k and nothing else.  No atomics, no host read-back.
// THE ONE COUPLING BETWEEN PIXELS (adaptive_connections_item below): with it an adaptive call traces the connections of a depth
//   whatever its other tiles do.  The product with the setting off drops them for a sub-batch (and a rank: each renders its own)
//   none of whose paths goes on — ASSUMED not to happen to a sub-batch that traces a rank's whole strips below max_depth; where it
//   does, "setting on, nothing retired" traces connections that "setting off" drops.
// PRESENT: a pixel is scaled by 1 / n_tile of its tile, a correctly rounded float32 division as the host's 1.0f / (float)n (0 for 0).
#pragma once

static_assert(NZ_TILE_Y == TILE && NZ_TILE_X % TILE == 0, "a noise tile is a row of whole slot tiles");

// the slot tile (index into the mask) of path slot `slot`
RT_FN uint32_t ad_slot_tile(const FrameView &fr, uint32_t slot)
{
	const uint32_t gl = fr.sgroup_log2;
	const uint32_t sgroup = fast_div(slot, fr.div_group); // (as slot_to_pixel)
	return (slot - sgroup * (fr.slots << gl)) >> (6u + gl);
}
// the noise tile of local pixel (x, yl)
RT_FN uint32_t ad_tile_of(uint32_t ntx, uint32_t x, uint32_t yl) { return (yl / NZ_TILE_Y) * ntx + x / NZ_TILE_X; }

RT_FN f4 ad_void_hit() { return mk4(1e34f, 0.0f, 0.0f, ubits((uint32_t)HIT_VOID)); }

// entry i of a per-lane primary wave: a retired tile's entry leaves its void record, an active one is extend_item<GEN_PT>'s.
// The mask byte is read per lane here — one byte load whose address is the same for a wave's 64 lanes, not the packet form's scalar
// load: this is the kernel of small launches (1-spp frames, refill without bit 3), and a lane with i >= count must read nothing
template <bool COUNT> RT_FN void extend_masked_item(const Params &p, const unsigned char *mask, uint32_t i, bool active, Ctx &ctx)
{
	if (active && !mask[ad_slot_tile(p.fr, i)])
	{
		p.wv.hit0[i] = ad_void_hit();
		active = false;
	}
	extend_item<GEN_PT, COUNT>(p, i, active, ctx);
}

RT_FN void resolve_adaptive_item(const Params &p, float *moments, const AdaptiveView &v, uint32_t li)
{
	const uint32_t t = ad_tile_of(v.ntx, li % p.fr.W, li / p.fr.W);
	if (!v.active[t])
		return; // (frozen: accumulator and moments; its slots hold nothing)
	resolve_noise_item(p, moments, v.n_tile[t], li);
}

RT_FN void present_adaptive_item(const Params &p, f4 *out, const AdaptiveView &v, int full, uint32_t li)
{
	const uint32_t n = v.n_tile[ad_tile_of(v.ntx, li % p.fr.W, li / p.fr.W)];
	present_item(p, out, n ? 1.0f / (float)n : 0.0f, full, li);
}

// nz_pixel_item with the tile's own sample count
RT_FN bool ad_noise_pixel_item(const NoiseView &v, const uint32_t *n_tile, uint32_t x, uint32_t yl, float &e)
{
	NoiseView w = v;
	if (x < v.W && yl < v.local_rows)
		w.n = n_tile[ad_tile_of((v.W + NZ_TILE_X - 1u) / NZ_TILE_X, x, yl)];
	return nz_pixel_item(w, x, yl, e);
}

// The connections of depth `depth` are traced only when a path of the launch's sub-batch went on to depth + 1 (connection_count,
// kernels.hip: the reference's host loop ends with the last wave that has rays, and its connections are never traced).  That is the
// one place where a pixel's light depends on other pixels.  A sub-batch that traces the whole strips of its rank is assumed to have a path that goes on
// below max_depth (see the header of this file), so the rule drops no connection there; the few active tiles of an adaptive call can be without one, and their pixels would then differ
// from the same pixels of a call that traces the whole frame.  So an adaptive call states what holds for the frame: where depth
// `depth` queued connections and no path went on, "one did" (ext, not the queue length ext_n: nothing is traced for it, and
// rfwhip_wait takes the mark out of the ray counts).  One thread, behind the shade launch of that depth on its stream.
RT_FN void adaptive_connections_item(WaveCounters *c, uint32_t depth)
{
	if (c->shadow_n[depth] && !c->ext[depth + 1u])
		c->ext[depth + 1u] = 1u;
}

// RESET / rfwhip_init
RT_FN void adaptive_reset_item(const AdaptiveView &v, uint32_t t)
{
	if (t >= v.count)
		return;
	v.n_tile[t] = 0u, v.active[t] = 1;
	const uint32_t ty = t / v.ntx, sx = (t - ty * v.ntx) * (NZ_TILE_X / TILE);
	for (uint32_t k = 0; k < NZ_TILE_X / TILE; k++)
		if (sx + k < v.tiles_x)
			v.mask[ty * v.tiles_x + sx + k] = 1;
}

// tile t after a call: `add` samples more where it is active; decide: the rule on the tile's record (which the metric has just written)
RT_FN void adaptive_step_item(const AdaptiveView &v, uint32_t add, bool decide, uint32_t t)
{
	if (t >= v.count || !v.active[t])
		return;
	const uint32_t n = v.n_tile[t] + add;
	v.n_tile[t] = n;
	if (decide && n >= v.min_samples && v.tiles[t].converged == v.tiles[t].pixels)
	{
		v.active[t] = 0;
		const uint32_t ty = t / v.ntx, sx = (t - ty * v.ntx) * (NZ_TILE_X / TILE);
		for (uint32_t k = 0; k < NZ_TILE_X / TILE; k++)
			if (sx + k < v.tiles_x)
				v.mask[ty * v.tiles_x + sx + k] = 0;
	}
}
