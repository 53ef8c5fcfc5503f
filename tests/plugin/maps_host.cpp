// maps_host.cpp — the setting material_maps through the plugin boundary: dlopen "HipRT.so", hand the rfw::RenderContext a scene whose
// front quad carries a white texture (alpha 255) and a mask in the RGB of an alpha map — what rfw::system hands over for such a
// material: the HasAlphaMap flag, the descriptor of slot 9 and texture id [10] — render one frame and compare it with the frame of a
// group driven through the C ABI directly with material_maps set to what RFWHIP_MATERIAL_MAPS says ("1": on; unset or "0": off).
// Prints what hiprtGetSetting answers for "material_maps" and "material_maps_on" and whether the two frames are equal byte for byte;
// writes the plugin's frame to <argv[2]>/plugin.rgba32f.  The reference group renders BEFORE the plugin is opened.
#include "host_common.h"

typedef int (*GetSettingFn)(rfw::RenderContext *, const char *, char *, size_t);

// the host's scene with the two textures and the front quad's maps
struct MapsScene
{
	SceneData s;
	uint32_t white[16], mask[16];
	rfw::TextureData tex[2];
	MapsScene() : s(glm::vec3{0.25f, 0.5f, 0.75f})
	{
		for (int i = 0; i < 16; i++)
		{
			white[i] = 0xFFFFFFFFu;
			const uint32_t g = ((i & 1) ^ ((i >> 2) & 1)) ? 0xF0u : 0x10u; // a checkerboard on both sides of 0.5
			mask[i] = 0xFF000000u | g << 16 | g << 8 | g;
		}
		std::memset(tex, 0, sizeof(tex));
		const uint32_t *data[2] = {white, mask};
		for (int k = 0; k < 2; k++)
			tex[k].type = RFWHIP_TEX_UINT, tex[k].width = 4, tex[k].height = 4, tex[k].texelCount = 16, tex[k].data = const_cast<uint32_t *>(data[k]);
		// (rough surfaces: the point light shows the front quad, and the back quad where the mask lets a path through)
		s.mat[0].parameters[0] = s.mat[1].parameters[0] = 0x807F0000u; // roughness 128, specular 127
		s.mat[0].parameters[2] = s.mat[1].parameters[2] = 0x7F00FF00u; // eta * 0.5 = 127, clearcoatGloss 255: the host material's defaults
		rfw::DeviceMaterial &m = s.mat[0];
		m.flags = 1u << 2 | 1u << 13; // HasDiffuseMap, HasAlphaMap
		for (int slot : {0, 9})
			m.map[slot].width = 4, m.map[slot].height = 4, m.map[slot].uscale = m.map[slot].vscale = 0x3C00; // 1.0 in binary16
		s.ids[0].texture[0] = 0, s.ids[0].texture[10] = 1;
		// uv 0 .. 1 across the front quad (triangles 0 2 1 and 0 3 2 of vertices (-1,-1) (1,-1) (1,1) (-1,1))
		s.tris[0].u0 = 0, s.tris[0].u1 = 1, s.tris[0].u2 = 1, s.tris[0].v0 = 0, s.tris[0].v1 = 1, s.tris[0].v2 = 0;
		s.tris[1].u0 = 0, s.tris[1].u1 = 0, s.tris[1].u2 = 1, s.tris[1].v0 = 0, s.tris[1].v1 = 1, s.tris[1].v2 = 1;
	}
};

static int reference(const MapsScene &m, bool on, std::vector<float> &want)
{
	rfwhip_group *g = nullptr;
	if (int r = reference_group(&g))
		return r;
	ABI(rfwhip_group_set_setting(g, "material_maps", on ? "1" : "0"));
	rfwhip_context *c = rfwhip_group_context(g, 0);
	if (int r = scene_abi(c, m.s))
		return r;
	ABI(rfwhip_set_textures(c, reinterpret_cast<const rfwhip_texture *>(m.tex), 2));
	ABI(rfwhip_group_update(g));
	const rfwhip_camera cam = pod(camera());
	ABI(rfwhip_group_render(g, &cam, RFWHIP_RESET));
	want.resize(size_t(W) * H * 4);
	ABI(rfwhip_group_read_framebuffer(g, want.data()));
	rfwhip_group_destroy(g);
	return 0;
}

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".", out = argc > 2 ? argv[2] : ".";
	const bool on = std::getenv("RFWHIP_MATERIAL_MAPS") && std::string(std::getenv("RFWHIP_MATERIAL_MAPS")) == "1";
	const bool valid = !std::getenv("RFWHIP_MATERIAL_MAPS") || on || std::string(std::getenv("RFWHIP_MATERIAL_MAPS")) == "0";
	MapsScene m;
	std::vector<float> want;
	if (valid) // (a value the plugin refuses ends in its constructor: nothing to compare with)
		if (int rc = reference(m, on, want))
			return rc;
	Plugin p;
	if (int r = p.open(dir, {"hiprtReadFramebuffer", "hiprtGetSetting"}))
		return r;
	auto read = (ReadFn)p.sym[0];
	auto get_setting = (GetSettingFn)p.sym[1];
	return drive(p, [&](rfw::RenderContext *ctx, int &rc) {
		GLuint tex = 0;
		ctx->init(&tex, W, H);
		ctx->set_sky(m.s.sky, 8, 4);
		ctx->set_textures({m.tex[0], m.tex[1]});
		ctx->set_materials({m.s.mat[0], m.s.mat[1]}, {m.s.ids[0], m.s.ids[1]});
		ctx->set_mesh(0, m.s.mesh);
		glm::mat4 M = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
		glm::mat3 N = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
		ctx->set_instance(0, 0, M, N);
		rfw::LightCount lc = {0, 1, 0, 0};
		ctx->set_lights(lc, nullptr, &m.s.pl, nullptr, nullptr);
		ctx->update();
		ctx->render_frame(camera(), rfw::Reset);
		std::vector<float> got(size_t(W) * H * 4);
		char setting[16] = "?", maps_on[16] = "?";
		if (read(ctx, got.data()) || get_setting(ctx, "material_maps", setting, sizeof(setting)) ||
			get_setting(ctx, "material_maps_on", maps_on, sizeof(maps_on)))
			rc = 4;
		std::printf("material_maps %s\nmaterial_maps_on %s\n", setting, maps_on);
		std::printf("equal %d\n", std::memcmp(got.data(), want.data(), got.size() * sizeof(float)) == 0 ? 1 : 0);
		if (int r = dump(out + "/plugin.rgba32f", got.data(), got.size() * sizeof(float)))
			rc = r;
		return 0;
	});
}
