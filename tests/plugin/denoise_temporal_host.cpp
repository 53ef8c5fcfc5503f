// denoise_temporal_host.cpp — the denoiser's temporal stage through the plugin boundary: dlopen "HipRT.so", drive the
// rfw::RenderContext through its VIRTUAL interface (get_settings must list "DENOISE_TEMPORAL" with "0" / "1"; DENOISE and
// DENOISE_TEMPORAL on; a camera that moves every frame, Reset every frame), and compare every image render_frame hands out
// (RFWHIP_FRAMES_IN_FLIGHT of the environment: frame k - n + 1) bit for bit with the images of a context driven through the C ABI
// directly (rfwhip_read_framebuffer after each render, denoise and denoise_temporal on).  The history follows the presented
// frames: with n frames in flight the plugin presents frames 0 .. FRAMES - n, each once, in order, as the C ABI context does.
// Compiled by tests/test_denoise_temporal_plugin_gpu.py against the restated interface header and librfwhip.so.
#include "rfw/restated_context.h"
#include "rfwhip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <vector>

typedef rfw::RenderContext *(*CreateFn)();
typedef void (*DestroyFn)(rfw::RenderContext *);
typedef int (*ReadFn)(rfw::RenderContext *, float *);

static const uint W = 96, H = 64;
static const int FRAMES = 6;

// the scene of plugin_host.cpp plus a second quad behind it (depth and normal edges for the filter) and a grey material
struct SceneData
{
	rfw::DeviceMaterial mat[2];
	rfw::MaterialTexIds ids[2];
	float verts[8][4] = {{-1, -1, 4, 1}, {1, -1, 4, 1}, {1, 1, 4, 1}, {-1, 1, 4, 1},
						 {-3, -3, 7, 1}, {3, -3, 6, 1}, {3, 3, 6, 1}, {-3, 3, 7, 1}};
	unsigned idx[4][3] = {{0, 2, 1}, {0, 3, 2}, {4, 6, 5}, {4, 7, 6}};
	rfw::Triangle tris[4];
	std::vector<glm::vec3> sky = std::vector<glm::vec3>(8 * 4, glm::vec3{0.25f, 0.5f, 0.75f});
	rfw::DevicePointLight pl;
	rfw::Mesh mesh;
	SceneData()
	{
		std::memset(mat, 0, sizeof(mat));
		std::memset(ids, 0xFF, sizeof(ids)); // no textures: every slot -1
		mat[0].diffuse[0] = mat[0].diffuse[1] = mat[0].diffuse[2] = 0x3800; // 0.5 in binary16
		mat[1].diffuse[0] = 0x3A00, mat[1].diffuse[1] = 0x3400, mat[1].diffuse[2] = 0x3000; // 0.75, 0.25, 0.125
		std::memset(tris, 0, sizeof(tris));
		for (int t = 0; t < 4; t++)
		{
			tris[t].lightTriIdx = -1, tris[t].material = t < 2 ? 0 : 1;
			tris[t].vN0[2] = tris[t].vN1[2] = tris[t].vN2[2] = tris[t].Nz = -1.0f;
		}
		std::memset(&pl, 0, sizeof(pl));
		pl.position[2] = 0.0f, pl.radiance[0] = pl.radiance[1] = pl.radiance[2] = 8.0f, pl.energy = std::sqrt(192.0f);
		mesh.vertices = &verts[0][0], mesh.normals = nullptr, mesh.texCoords = nullptr, mesh.triangles = tris;
		mesh.indices = &idx[0][0], mesh.vertexCount = 8, mesh.triangleCount = 4;
	}
};

static rfw::Camera camera(int k)
{
	rfw::Camera cam;
	std::memset(&cam, 0, sizeof(cam));
	cam.position.x = 0.02f * (float)k; // a slow pan
	cam.direction.z = 1.0f, cam.focalDistance = 5.0f, cam.FOV = 40.0f, cam.aspectRatio = float(W) / H, cam.clampValue = 10.0f;
	cam.pixelCount = glm::ivec2{int(W), int(H)};
	return cam;
}

#define ABI(call)                                                                    \
	do                                                                               \
	{                                                                                \
		if ((call) != RFWHIP_OK)                                                     \
		{                                                                            \
			std::fprintf(stderr, "%s failed: %s\n", #call, rfwhip_last_error());     \
			return 6;                                                                \
		}                                                                            \
	} while (0)

// the C ABI's denoised images of frames 0 .. FRAMES - 1 (and the raw image of the last one)
static int reference(const SceneData &s, std::vector<std::vector<float>> &den, std::vector<float> &raw)
{
	rfwhip_context *c = nullptr;
	ABI(rfwhip_create(0, 0, 1, &c));
	ABI(rfwhip_init(c, W, H));
	ABI(rfwhip_set_setting(c, "integrator", "pt"));
	ABI(rfwhip_set_setting(c, "denoise", "1"));
	ABI(rfwhip_set_setting(c, "denoise_temporal", "1"));
	ABI(rfwhip_set_sky(c, reinterpret_cast<const float *>(s.sky.data()), 8, 4));
	ABI(rfwhip_set_textures(c, nullptr, 0));
	ABI(rfwhip_set_materials(c, reinterpret_cast<const rfwhip_material *>(s.mat), reinterpret_cast<const rfwhip_material_tex_ids *>(s.ids), 2));
	ABI(rfwhip_set_mesh(c, 0, reinterpret_cast<const rfwhip_mesh *>(&s.mesh)));
	const float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, N[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	ABI(rfwhip_set_instance(c, 0, 0, M, N));
	rfwhip_light_count lc = {0, 1, 0, 0};
	ABI(rfwhip_set_lights(c, lc, nullptr, reinterpret_cast<const rfwhip_point_light *>(&s.pl), nullptr, nullptr));
	ABI(rfwhip_update(c));
	den.assign(FRAMES, std::vector<float>(size_t(W) * H * 4));
	for (int k = 0; k < FRAMES; k++)
	{
		const rfw::Camera cam = camera(k);
		rfwhip_camera pod;
		std::memcpy(&pod, &cam, sizeof(pod));
		ABI(rfwhip_render(c, &pod, RFWHIP_RESET));
		ABI(rfwhip_wait(c));
		ABI(rfwhip_read_framebuffer(c, den[k].data()));
	}
	// the last frame's spatial-only filter: the temporal output must differ from it
	raw.assign(size_t(W) * H * 4, 0.0f);
	ABI(rfwhip_set_setting(c, "denoise", "0"));
	ABI(rfwhip_read_framebuffer(c, raw.data()));
	ABI(rfwhip_denoise_image(c, raw.data(), raw.data()));
	rfwhip_destroy(c);
	return 0;
}

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".";
	const int in_flight = std::getenv("RFWHIP_FRAMES_IN_FLIGHT") ? std::max(1, std::atoi(std::getenv("RFWHIP_FRAMES_IN_FLIGHT"))) : 1;
	SceneData s;
	std::vector<std::vector<float>> want;
	std::vector<float> raw;
	if (int rc = reference(s, want, raw))
		return rc;
	void *h = dlopen((dir + "/HipRT.so").c_str(), RTLD_NOW);
	if (!h)
	{
		std::fprintf(stderr, "dlopen failed: %s\n", dlerror());
		return 2;
	}
	auto create = (CreateFn)dlsym(h, "createRenderContext");
	auto destroy = (DestroyFn)dlsym(h, "destroyRenderContext");
	auto readfb = (ReadFn)dlsym(h, "hiprtReadFramebuffer");
	if (!create || !destroy || !readfb)
		return 3;
	int rc = 0;
	try
	{
		rfw::RenderContext *ctx = create();
		GLuint tex = 0;
		ctx->init(&tex, W, H);
		const rfw::AvailableRenderSettings st = ctx->get_settings();
		int listed = 0;
		for (size_t i = 0; i < st.settingKeys.size(); i++)
			if (st.settingKeys[i] == "DENOISE_TEMPORAL" && i < st.settingValues.size() && st.settingValues[i] == std::vector<std::string>{"0", "1"})
				listed = 1;
		std::printf("listed %d\n", listed);
		ctx->set_setting(rfw::RenderSetting("DENOISE", "1"));
		ctx->set_setting(rfw::RenderSetting("DENOISE_TEMPORAL", "1"));
		ctx->set_sky(s.sky, 8, 4);
		ctx->set_textures({});
		ctx->set_materials({s.mat[0], s.mat[1]}, {s.ids[0], s.ids[1]});
		ctx->set_mesh(0, s.mesh);
		glm::mat4 M = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
		glm::mat3 N = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
		ctx->set_instance(0, 0, M, N);
		rfw::LightCount lc = {0, 1, 0, 0};
		ctx->set_lights(lc, nullptr, &s.pl, nullptr, nullptr);
		ctx->update();
		std::vector<float> img(size_t(W) * H * 4);
		int equal = 0;
		for (int k = 0; k < FRAMES; k++)
		{
			ctx->render_frame(camera(k), rfw::Reset);
			if (readfb(ctx, img.data()) != 0)
				rc = 4;
			// what render_frame hands out with n frames in flight: frame k - n + 1 (frame 0 until there is an older one)
			const int shown = std::max(0, k - in_flight + 1);
			equal += std::memcmp(img.data(), want[(size_t)shown].data(), img.size() * sizeof(float)) == 0;
		}
		std::printf("frames %d equal %d\n", FRAMES, equal);
		std::printf("differs_from_spatial %d\n", std::memcmp(want.back().data(), raw.data(), raw.size() * sizeof(float)) != 0 ? 1 : 0);
		ctx->cleanup();
		destroy(ctx);
	}
	catch (const std::exception &e)
	{
		std::fprintf(stderr, "exception: %s\n", e.what());
		rc = 5;
	}
	dlclose(h);
	return rc;
}
