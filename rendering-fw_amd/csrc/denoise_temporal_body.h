// denoise_temporal_body.h — the body of the temporal stage's item, included by its two functions in denoise.h: dn_temporal_item
// (DN_BODY_MOTION 0, the default) and dn_temporal_motion_item (DN_BODY_MOTION 1, setting "denoise_motion").  In scope there: d, t,
// img, var, i and, with DN_BODY_MOTION, m (DnMotion).  Spelled out per function with the preprocessor, as shade_pt_body.h is per
// kernel: the default item's code, and with it k_dn_temporal, stays exactly what it was.
// (no include guard: it is included once per function)
	const f4 gp = d.gb[i];
	if (gp.y < 0.0f)
	{
		d.hist[i] = mk4(0.0f, 0.0f, 0.0f, 0.0f); // (never read: P's guide at an invalid pixel fails every tap)
		t.mom_out[2 * i] = 0.0f, t.mom_out[2 * i + 1] = 0.0f, t.n_out[i] = 0.0f;
#if DN_BODY_MOTION
		if (m.dump)
			dn_motion_dump(m, i, DN_M_INVALID, mk3(0, 0, 0), mk3(0, 0, 0));
#endif
		return;
	}
	const uint32_t x = i % d.W, y = i / d.W;
	const f4 I = img[i];
	const float l = I.w;
	// the consistent bilinear taps of X in P (fixed order: (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1))
	float wq[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ws = 0.0f;
	uint32_t qi[4] = {0u, 0u, 0u, 0u};
#if DN_BODY_MOTION
	uint32_t mstate = DN_M_RESTART; // (what m.dump reports; every valid pixel while the history is not usable)
	f3 mX = mk3(0, 0, 0), mn = mk3(0, 0, 0);
#endif
	if (t.usable)
	{
		f3 O, D;
		pt_center_ray(t.cam, t.fr, x, y, O, D);
#if DN_BODY_MOTION
		// a pixel of a MOVED instance takes the previous position of its surface point and its normal carried back to P
		f3 X = O + D * gp.y, np = dn_oct_decode(fbits(gp.x));
		const uint32_t id = t.id[i];
		bool same = id < t.n_inst && t.inst_ver[id] <= t.pscene; // (the instance has not changed since P)
		mstate = same ? DN_M_STILL : DN_M_RESTART;
		if (!same && id < t.n_inst && m.inst[id].state == DN_M_MOVED)
		{
			mstate = DN_M_MOVED;
			same = dn_motion_point(m.inst[id], m.surf[i], X, np); // (false: a degenerate triangle, the pixel is fresh)
		}
		if (mstate != DN_M_RESTART)
			mX = X, mn = np;
		const f3 e = X - t.pcam.pos;
#else
		const f3 X = O + D * gp.y, e = X - t.pcam.pos;
#endif
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
#if !DN_BODY_MOTION
				const uint32_t id = t.id[i];
				const bool same = id < t.n_inst && t.inst_ver[id] <= t.pscene; // (the instance has not changed since P)
				const f3 np = dn_oct_decode(fbits(gp.x));
#endif
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
#if DN_BODY_MOTION
	if (m.dump)
		dn_motion_dump(m, i, mstate, mX, mn);
#endif
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
