// denoise.h — the work items of the denoiser of the presented image (setting "denoise", include/rfwhip.h): a guide pass and
// SVGF's filter (Schied et al., HPG 2017): the spatial a-trous passes and its temporal stage.  Included by kernels.hip inside namespace rtk,
// after the other work items: the device kernels (kernels.hip) and the host emulation (kernels_emu.inc) run the same items.
//
// Guides, per pixel of the full W x H image (one centre ray from the lens centre, the closest-hit traversal of the path tracer):
//   ga = albedo (material colour after the texture layers, pt_textures), w = 1 valid / 0 invalid
//   gb = octahedral normal (two snorm16 in the bits of x: the shading normal after normal maps, facing the camera), z = distance
//        along the ray to the surface (-1 = invalid), dz/dx, dz/dy (central differences; one-sided at borders / invalid neighbours)
// A pixel is invalid when its ray misses, hits an emitter (a colour component > 1, pt_shade), or passes more than DN_MAX_ALPHA
// alpha-tested layers (the path tracer's pass-through: the ray goes on from I + 1e-5 D).
// Filter (valid pixels; invalid ones are copied bit for bit and never used as neighbours):
//   demodulate  I = c / max(albedo, 1e-3), l = lum(I); var = weighted variance of l over the valid 3x3 neighbours (weights w_z w_n)
//   pass i      step s = 2^i, 5x5 taps q = p + s (dx, dy), w = h(dx) h(dy) w_z w_n w_l, h = (1, 4, 6, 4, 1) / 16
//               w_z = exp(-|z_p - z_q| / (sigma_z |s (dx, dy) . grad z_p| + 1e-4)), w_n = max(0, n_p . n_q)^sigma_n,
//               w_l = exp(-|l_p - l_q| / (sigma_l sqrt(g3x3(var)_p) + 1e-10)), g3x3 = (1, 2, 1) / 4 x (1, 2, 1) / 4 over valid taps
//               I' = sum w I_q / sum w, var' = sum w^2 var_q / (sum w)^2, l' = lum(I')
//   remodulate  (last pass) out = I' max(albedo, 1e-3), out.w = c.w
// Fixed tap order, no atomics: the output depends on the input image and the guides only.
// Temporal stage (setting "denoise_temporal"; SVGF's reprojected history): dn_temporal_item follows the demodulation once per
// presented frame F.  It reprojects p's guide point X = pos_F + z_p D_p into the previous presented frame P (bilinear taps, each
// kept when it is consistent: inside, valid, the same unchanged instance, depth and normal within DN_T_*), blends I and the
// luminance moments with the history (n = min(n_P + 1, 64), a = max(alpha, 1 / n)) and takes var = max(0, mu2 - mu1^2) once
// n >= 4 (the 3x3 estimate before).  Pass 0 writes the colour history (its demodulated output).  A fresh pixel (no consistent
// tap, or no usable history) reads no history and gives the spatial filter's values bit for bit.
#pragma once

constexpr int DN_MAX_ALPHA = 8;			// alpha-tested layers a guide ray passes before the pixel is called invalid
constexpr float DN_ALBEDO_MIN = 1e-3f;	// demodulation floor per channel
constexpr int DN_TILE_X = 16, DN_TILE_Y = 16; // pixels of a 256-thread workgroup: 2 x 2 tiles of 8 x 8, one per wave64
// temporal stage (include/rfwhip.h "denoise_temporal" names the same constants)
constexpr float DN_T_DEPTH_GRAD = 2.0f;	 // depth test: |z_P(q) - |X - pos_P|| <= 2 (|dz/dx| + |dz/dy|) + 0.01 |X - pos_P|
constexpr float DN_T_DEPTH_REL = 0.01f;
constexpr float DN_T_NORMAL = 0.9f;		 // normal test: n_p . n_P(q) >= 0.9
constexpr float DN_T_MIN_WEIGHT = 0.01f; // a pixel whose consistent bilinear weights sum below this starts fresh
constexpr float DN_T_MAX_N = 64.0f;		 // history length cap
constexpr float DN_T_VAR_N = 3.99f;		 // from this history length on (4, less a margin for the rounding of the interpolated length:
										 // n_P is a weighted sum), the variance comes from the moments
constexpr uint32_t DN_NO_INST = 0xFFFFFFFFu; // instance id of an invalid guide pixel

RT_FN float dn_lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

RT_FN float dn_sign(float v) { return v < 0.0f ? -1.0f : 1.0f; }
RT_FN uint32_t dn_oct_encode(f3 n)
{
	const float s = fabsf(n.x) + fabsf(n.y) + fabsf(n.z);
	float px = n.x / s, py = n.y / s;
	if (n.z < 0.0f)
	{
		const float ox = (1.0f - fabsf(py)) * dn_sign(px), oy = (1.0f - fabsf(px)) * dn_sign(py);
		px = ox, py = oy;
	}
	const int qx = (int)rintf(fminf(fmaxf(px, -1.0f), 1.0f) * 32767.0f), qy = (int)rintf(fminf(fmaxf(py, -1.0f), 1.0f) * 32767.0f);
	return ((uint32_t)qx & 0xFFFFu) | ((uint32_t)qy << 16);
}
RT_FN f3 dn_oct_decode(uint32_t e)
{
	float x = (float)(int16_t)(e & 0xFFFFu) * (1.0f / 32767.0f), y = (float)(int16_t)(e >> 16) * (1.0f / 32767.0f);
	const float z = 1.0f - fabsf(x) - fabsf(y);
	if (z < 0.0f)
	{
		const float ox = (1.0f - fabsf(y)) * dn_sign(x), oy = (1.0f - fabsf(x)) * dn_sign(y);
		x = ox, y = oy;
	}
	const float inv = 1.0f / sqrtf(x * x + y * y + z * z);
	return mk3(x * inv, y * inv, z * inv);
}

// pixel of thread t of workgroup (bx, by): the 8 x 8 tile of wave t / 64, row-major inside it
RT_FN bool dn_pixel(uint32_t bx, uint32_t by, uint32_t t, uint32_t W, uint32_t H, uint32_t &i)
{
	const uint32_t wave = t >> 6, lane = t & 63u;
	const uint32_t x = bx * DN_TILE_X + (wave & 1u) * TILE + (lane & 7u), y = by * DN_TILE_Y + (wave >> 1) * TILE + (lane >> 3);
	i = y * W + x;
	return x < W && y < H;
}

// ---- guide pass ---------------------------------------------------------------------------------------------------------
RT_FN void dn_guide_item(const Params &p, const DnView &d, uint32_t i, const TravStack &stk)
{
	const uint32_t x = i % d.W, y = i / d.W;
	f3 O, D;
	pt_center_ray(p.cam, p.fr, x, y, O, D);
	f3 albedo = mk3(0, 0, 0), n = mk3(0, 0, 1);
	float z = 0.0f;
	bool valid = false;
	uint32_t inst = DN_NO_INST;
	for (int layer = 0; layer <= DN_MAX_ALPHA; layer++)
	{
		Hit h;
		TStat st;
		st.inner = 0, st.tris = 0, st.lds = 0;
		trace<false, false>(p.sc, O, D, 1e-5f, 1e34f, h, stk, st);
		if (h.prim < 0)
			break;
		Surface sf;
		pt_surface(p.sc, h, sf);
		f3 color = material_color(*sf.mat), iN = sf.iN;
		bool alpha_skip = false;
		if (p.textured && pt_has_textures(p.sc, sf))
			pt_textures(p.sc, p.cam, D, h.t, sf, color, iN, alpha_skip);
		z += h.t;
		if (alpha_skip)
		{
			// the path tracer's pass-through (pt_shade): on from I + 1e-5 D in the same direction
			const f3 I = O + D * h.t;
			O = I + D * 1e-5f;
			z += 1e-5f;
			continue;
		}
		if (!(color.x > 1.0f || color.y > 1.0f || color.z > 1.0f)) // (an emitter ends the path: pt_shade)
		{
			albedo = color;
			n = iN * ((dot(D, sf.N) > 0.0f) ? -1.0f : 1.0f);
			valid = true;
			inst = (uint32_t)h.inst;
		}
		break;
	}
	d.ga[i] = mk4(albedo.x, albedo.y, albedo.z, valid ? 1.0f : 0.0f);
	d.gb[i] = mk4(ubits(dn_oct_encode(n)), valid ? z : -1.0f, 0.0f, 0.0f);
	if (d.id) // (the temporal stage's instance test)
		d.id[i] = inst;
}

// screen-space depth gradient (a second kernel: it reads the neighbours' z); writes gb[i].z / .w only
RT_FN void dn_gradient_item(const DnView &d, uint32_t i)
{
	const uint32_t x = i % d.W, y = i / d.W;
	const float z = d.gb[i].y;
	if (z < 0.0f)
		return;
	auto zq = [&](int qx, int qy) -> float {
		if (qx < 0 || qy < 0 || qx >= (int)d.W || qy >= (int)d.H)
			return -1.0f;
		return d.gb[(uint32_t)qy * d.W + (uint32_t)qx].y;
	};
	auto diff = [&](float zm, float zp) -> float {
		if (zm >= 0.0f && zp >= 0.0f)
			return (zp - zm) * 0.5f;
		if (zp >= 0.0f)
			return zp - z;
		if (zm >= 0.0f)
			return z - zm;
		return 0.0f;
	};
	float *const g = (float *)&d.gb[i];
	g[2] = diff(zq((int)x - 1, (int)y), zq((int)x + 1, (int)y));
	g[3] = diff(zq((int)x, (int)y - 1), zq((int)x, (int)y + 1));
}

// ---- filter -------------------------------------------------------------------------------------------------------------
RT_FN float dn_w_z(const f4 &gp, const f4 &gq, float sigma_z, int sdx, int sdy)
{
	return expf(-fabsf(gp.y - gq.y) / (sigma_z * fabsf((float)sdx * gp.z + (float)sdy * gp.w) + 1e-4f));
}
RT_FN float dn_w_n(f3 np, f3 nq, float sigma_n) { return powf(fmaxf(0.0f, dot(np, nq)), sigma_n); }

// demodulation + the initial variance, into img (I, l) / var
RT_FN void dn_demod_item(const DnView &d, f4 *img, float *var, uint32_t i)
{
	const f4 gp = d.gb[i];
	if (gp.y < 0.0f)
		return;
	const int x = (int)(i % d.W), y = (int)(i / d.W);
	const f3 np = dn_oct_decode(fbits(gp.x));
	float w[9], l[9], sw = 0.0f, sl = 0.0f;
	for (int dy = -1; dy <= 1; dy++)
		for (int dx = -1; dx <= 1; dx++)
		{
			const int k = (dy + 1) * 3 + dx + 1, qx = x + dx, qy = y + dy;
			w[k] = 0.0f, l[k] = 0.0f;
			if (qx < 0 || qy < 0 || qx >= (int)d.W || qy >= (int)d.H)
				continue;
			const uint32_t q = (uint32_t)qy * d.W + (uint32_t)qx;
			const f4 gq = d.gb[q];
			if (gq.y < 0.0f)
				continue;
			const f4 a = d.ga[q], c = d.in[q];
			const float ir = c.x / fmaxf(a.x, DN_ALBEDO_MIN), ig = c.y / fmaxf(a.y, DN_ALBEDO_MIN), ib = c.z / fmaxf(a.z, DN_ALBEDO_MIN);
			l[k] = dn_lum(ir, ig, ib);
			w[k] = dn_w_z(gp, gq, d.sigma_z, dx, dy) * dn_w_n(np, dn_oct_decode(fbits(gq.x)), d.sigma_n);
			sw += w[k], sl += w[k] * l[k];
			if (k == 4)
				img[i] = mk4(ir, ig, ib, l[k]);
		}
	const float mean = sl / sw;
	float v = 0.0f;
	for (int k = 0; k < 9; k++)
		v += w[k] * (l[k] - mean) * (l[k] - mean);
	var[i] = v / sw;
}

// ---- temporal stage (after dn_demod_item when "denoise_temporal" is on) -----------------------------------------------------------
// The demodulation has written I, l and the 3x3 variance into img / var; this reprojects pixel i into the previous presented frame,
// blends with its history and chooses the variance, in place: img (I~, lum(I~)) / var; the moments and the history length into
// t.mom_out / t.n_out.  A fresh pixel leaves img / var as the demodulation wrote them: the spatial filter's values, bit for bit.
// Invalid pixels store n = 0.  (Reads and writes pixel i of img / var only.)
RT_FN void dn_temporal_item(const DnView &d, const DnTemporal &t, f4 *img, float *var, uint32_t i)
{
	const f4 gp = d.gb[i];
	if (gp.y < 0.0f)
	{
		d.hist[i] = mk4(0.0f, 0.0f, 0.0f, 0.0f); // (never read: P's guide at an invalid pixel fails every tap)
		t.mom_out[2 * i] = 0.0f, t.mom_out[2 * i + 1] = 0.0f, t.n_out[i] = 0.0f;
		return;
	}
	const uint32_t x = i % d.W, y = i / d.W;
	const f4 I = img[i];
	const float l = I.w;
	// the consistent bilinear taps of X in P (fixed order: (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1))
	float wq[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ws = 0.0f;
	uint32_t qi[4] = {0u, 0u, 0u, 0u};
	if (t.usable)
	{
		f3 O, D;
		pt_center_ray(t.cam, t.fr, x, y, O, D);
		const f3 X = O + D * gp.y, e = X - t.pcam.pos;
		const f3 pn = cross(t.pcam.right, t.pcam.up);
		const float s = dot(t.pcam.p1 - t.pcam.pos, pn) / dot(e, pn); // the ray pos_P -> X meets P's image plane at pos_P + s e
		if (s > 0.0f)
		{
			const f3 Q = t.pcam.pos + e * s - t.pcam.p1, R = t.pcam.right, U = t.pcam.up;
			const float rr = dot(R, R), ru = dot(R, U), uu = dot(U, U), qr = dot(Q, R), qu = dot(Q, U);
			const float det = rr * uu - ru * ru;
			const float xf = (qr * uu - qu * ru) / det * (float)d.W - 0.5f, yf = (qu * rr - qr * ru) / det * (float)d.H - 0.5f;
			if (xf > -1.0f && xf < (float)d.W && yf > -1.0f && yf < (float)d.H) // (false for NaN)
			{
				const float fx0 = floorf(xf), fy0 = floorf(yf), fx = xf - fx0, fy = yf - fy0;
				const int x0 = (int)fx0, y0 = (int)fy0;
				const float dist = length(e);
				const uint32_t id = t.id[i];
				const bool same = id < t.n_inst && t.inst_ver[id] <= t.pscene; // (the instance has not changed since P)
				const f3 np = dn_oct_decode(fbits(gp.x));
				for (int k = 0; k < 4; k++)
				{
					const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
					const float bw = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
					if (!same || bw <= 0.0f || qx < 0 || qy < 0 || qx >= (int)d.W || qy >= (int)d.H)
						continue;
					const uint32_t q = (uint32_t)qy * d.W + (uint32_t)qx;
					const f4 gq = t.pgb[q];
					if (gq.y < 0.0f || t.pid[q] != id)
						continue;
					if (fabsf(gq.y - dist) > DN_T_DEPTH_GRAD * (fabsf(gq.z) + fabsf(gq.w)) + DN_T_DEPTH_REL * dist)
						continue;
					if (dot(np, dn_oct_decode(fbits(gq.x))) < DN_T_NORMAL)
						continue;
					wq[k] = bw, qi[k] = q, ws += bw;
				}
			}
		}
	}
	if (!(ws >= DN_T_MIN_WEIGHT))
	{
		// fresh: no history is read, img / var stay the demodulation's
		t.mom_out[2 * i] = l, t.mom_out[2 * i + 1] = l * l, t.n_out[i] = 1.0f;
		return;
	}
	const float inv = 1.0f / ws;
	float hr = 0.0f, hg = 0.0f, hb = 0.0f, h1 = 0.0f, h2 = 0.0f, hn = 0.0f;
	for (int k = 0; k < 4; k++)
	{
		if (wq[k] == 0.0f)
			continue;
		const float w = wq[k] * inv;
		const f4 hc = t.col_in[qi[k]];
		hr += w * hc.x, hg += w * hc.y, hb += w * hc.z;
		h1 += w * t.mom_in[2 * qi[k]], h2 += w * t.mom_in[2 * qi[k] + 1], hn += w * t.n_in[qi[k]];
	}
	const float n = fminf(hn + 1.0f, DN_T_MAX_N);
	const float al = fmaxf(t.alpha, 1.0f / n), bl = 1.0f - al;
	const float r = bl * hr + al * I.x, g = bl * hg + al * I.y, b = bl * hb + al * I.z;
	const float m1 = bl * h1 + al * l, m2 = bl * h2 + al * (l * l);
	img[i] = mk4(r, g, b, dn_lum(r, g, b));
	if (n >= DN_T_VAR_N) // (before: the 3x3 estimate the demodulation wrote)
		var[i] = fmaxf(0.0f, m2 - m1 * m1);
	t.mom_out[2 * i] = m1, t.mom_out[2 * i + 1] = m2, t.n_out[i] = n;
}

// one a-trous pass of step `step`: src / vsrc -> dst / vdst, or (last) the remodulated image into d.out (may be d.in)
RT_FN void dn_pass_item(const DnView &d, uint32_t step, bool last, const f4 *src, const float *vsrc, f4 *dst, float *vdst, uint32_t i)
{
	const f4 gp = d.gb[i];
	if (gp.y < 0.0f)
	{
		if (last)
			d.out[i] = d.in[i];
		return;
	}
	const int x = (int)(i % d.W), y = (int)(i / d.W);
	// the luminance edge's scale: the variance blurred over the valid 3 x 3 neighbours
	float gv = 0.0f, gw = 0.0f;
	for (int dy = -1; dy <= 1; dy++)
		for (int dx = -1; dx <= 1; dx++)
		{
			const int qx = x + dx, qy = y + dy;
			if (qx < 0 || qy < 0 || qx >= (int)d.W || qy >= (int)d.H)
				continue;
			const uint32_t q = (uint32_t)qy * d.W + (uint32_t)qx;
			if (d.gb[q].y < 0.0f)
				continue;
			const float k = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
			gv += k * vsrc[q], gw += k;
		}
	const float inv_l = 1.0f / (d.sigma_l * sqrtf(gv / gw) + 1e-10f);
	const f3 np = dn_oct_decode(fbits(gp.x));
	const float lp = src[i].w;
	const float h[5] = {1.0f / 16.0f, 4.0f / 16.0f, 6.0f / 16.0f, 4.0f / 16.0f, 1.0f / 16.0f};
	float sw = 0.0f, sv = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
	for (int dy = -2; dy <= 2; dy++)
		for (int dx = -2; dx <= 2; dx++)
		{
			const int sdx = (int)step * dx, sdy = (int)step * dy, qx = x + sdx, qy = y + sdy;
			if (qx < 0 || qy < 0 || qx >= (int)d.W || qy >= (int)d.H)
				continue;
			const uint32_t q = (uint32_t)qy * d.W + (uint32_t)qx;
			const f4 gq = d.gb[q];
			if (gq.y < 0.0f)
				continue;
			const f4 iq = src[q];
			const float w = h[dx + 2] * h[dy + 2] * dn_w_z(gp, gq, d.sigma_z, sdx, sdy) * dn_w_n(np, dn_oct_decode(fbits(gq.x)), d.sigma_n) *
							expf(-fabsf(lp - iq.w) * inv_l);
			sw += w, sr += w * iq.x, sg += w * iq.y, sb += w * iq.z;
			sv += w * w * vsrc[q];
		}
	const float inv = 1.0f / sw;
	const float r = sr * inv, g = sg * inv, b = sb * inv;
	if (last)
	{
		const f4 a = d.ga[i], c = d.in[i];
		d.out[i] = mk4(r * fmaxf(a.x, DN_ALBEDO_MIN), g * fmaxf(a.y, DN_ALBEDO_MIN), b * fmaxf(a.z, DN_ALBEDO_MIN), c.w);
	}
	else
	{
		dst[i] = mk4(r, g, b, dn_lum(r, g, b));
		vdst[i] = sv * inv * inv;
	}
	if (step == 1u && d.hist) // (the temporal stage: pass 0's demodulated output is the colour history)
		d.hist[i] = mk4(r, g, b, dn_lum(r, g, b));
}
