// denoise_guide_body.h — the body of the denoiser's guide item, included by its two functions in denoise.h: dn_guide_item
// (DN_BODY_SURF 0, the default) and dn_guide_surf_item (DN_BODY_SURF 1, setting "denoise_motion": the kept hit's primitive and
// barycentrics also go into surf[i] = (prim, u, v, 0); prim = -1 at an invalid pixel); dn_guide_maps_item (DN_BODY_MAPS 1, setting
// "material_maps": the alpha mask passes the ray through as MF_ALPHA does; surf may be null).  In scope there: p, d, i, stk and, with
// DN_BODY_SURF, surf.  Spelled out per function with the preprocessor, as shade_pt_body.h is per kernel: the default item's code,
// and with it k_dn_guides, stays exactly what it was.
// (no include guard: it is included once per function)
	const uint32_t x = i % d.W, y = i / d.W;
	f3 O, D;
	pt_center_ray(p.cam, p.fr, x, y, O, D);
	f3 albedo = mk3(0, 0, 0), n = mk3(0, 0, 1);
	float z = 0.0f;
	bool valid = false;
	uint32_t inst = DN_NO_INST;
#if DN_BODY_SURF
	uint32_t sprim = 0xFFFFFFFFu; // (no kept hit: the pixel is invalid)
	float su = 0.0f, sv = 0.0f;
#endif
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
#if DN_BODY_MAPS
		if (!alpha_skip)
		{
			float a;
			alpha_skip = pt_maps_alpha(p.sc, p.cam, D, h.t, sf, a);
		}
#endif
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
#if DN_BODY_SURF
			sprim = (uint32_t)h.prim, su = h.u, sv = h.v;
#endif
		}
		break;
	}
	d.ga[i] = mk4(albedo.x, albedo.y, albedo.z, valid ? 1.0f : 0.0f);
	d.gb[i] = mk4(ubits(dn_oct_encode(n)), valid ? z : -1.0f, 0.0f, 0.0f);
	if (d.id) // (the temporal stage's instance test)
		d.id[i] = inst;
#if DN_BODY_SURF
#if DN_BODY_MAPS
	if (surf)
#endif
	surf[i] = mk4(ubits(sprim), su, sv, 0.0f);
#endif
