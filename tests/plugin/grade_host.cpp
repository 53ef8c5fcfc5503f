// grade_host.cpp — colour grading through the plugin boundary: dlopen "HipRT.so" with RFWHIP_DISPLAY and the RFWHIP_GRADE* /
// RFWHIP_DITHER variables the test sets in the environment, drive the rfw::RenderContext through its virtual interface for one frame
// and write what hiprtReadDisplay returns to <out>/plugin.rgba8.  Beside it, from a group driven through the C ABI directly on the
// same scene WITHOUT any grading setting touched: the linear image of the same frame (<out>/abi.f32, W x H float4) and its ungraded
// display bytes (<out>/abi.rgba8).  tests/test_display_grade_plugin_gpu.py shows abi.f32 through the Python host with the same
// settings and the same .cube file and asks for equal bytes.  The plugin is created FIRST: a value it refuses ends the program
// (exit status 5, the message on stderr) before anything renders.  Compiled by the test against the restated interface header and
// librfwhip.so.
#include "rfw/restated_context.h"
#include "rfwhip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <string>
#include <vector>

typedef rfw::RenderContext *(*CreateFn)();
typedef void (*DestroyFn)(rfw::RenderContext *);
typedef int (*ReadFn)(rfw::RenderContext *, uint8_t *);

static const uint W = 96, H = 64;

// the scene of exposure_host.cpp under a sky far above display white: it shows left and right of the back quad and bleeds over its edges
struct SceneData
{
	rfw::DeviceMaterial mat[2];
	rfw::MaterialTexIds ids[2];
	float verts[8][4] = {{-1, -1, 4, 1}, {1, -1, 4, 1}, {1, 1, 4, 1}, {-1, 1, 4, 1},
						 {-3, -3, 7, 1}, {3, -3, 6, 1}, {3, 3, 6, 1}, {-3, 3, 7, 1}};
	unsigned idx[4][3] = {{0, 2, 1}, {0, 3, 2}, {4, 6, 5}, {4, 7, 6}};
	rfw::Triangle tris[4];
	std::vector<glm::vec3> sky = std::vector<glm::vec3>(8 * 4, glm::vec3{2.0f, 4.0f, 8.0f});
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

static rfw::Camera camera()
{
	rfw::Camera cam;
	std::memset(&cam, 0, sizeof(cam));
	cam.direction.z = 1.0f, cam.focalDistance = 5.0f, cam.FOV = 40.0f, cam.aspectRatio = float(W) / H, cam.clampValue = 10.0f;
	cam.pixelCount = glm::ivec2{int(W), int(H)};
	cam.brightness = 0.05f, cam.contrast = 1.0f; // Camera.cpp:8-9
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

static int dump(const std::string &path, const void *data, size_t bytes)
{
	FILE *f = std::fopen(path.c_str(), "wb");
	if (!f || std::fwrite(data, 1, bytes, f) != bytes)
	{
		std::fprintf(stderr, "cannot write %s\n", path.c_str());
		return 7;
	}
	std::fclose(f);
	return 0;
}

// the C ABI's frame 0 without grading: the linear image and its display bytes
static int reference(const SceneData &s, const char *tonemap, const std::string &out)
{
	rfwhip_group *g = nullptr;
	const int device = 0;
	ABI(rfwhip_group_create(&device, 1, RFWHIP_TRANSPORT_AUTO, &g));
	rfwhip_context *c = rfwhip_group_context(g, 0);
	ABI(rfwhip_group_init(g, W, H));
	ABI(rfwhip_group_set_setting(g, "integrator", "pt"));
	ABI(rfwhip_group_set_setting(g, "display_tonemap", tonemap));
	ABI(rfwhip_set_sky(c, reinterpret_cast<const float *>(s.sky.data()), 8, 4));
	ABI(rfwhip_set_textures(c, nullptr, 0));
	ABI(rfwhip_set_materials(c, reinterpret_cast<const rfwhip_material *>(s.mat), reinterpret_cast<const rfwhip_material_tex_ids *>(s.ids), 2));
	ABI(rfwhip_set_mesh(c, 0, reinterpret_cast<const rfwhip_mesh *>(&s.mesh)));
	const float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, N[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	ABI(rfwhip_set_instance(c, 0, 0, M, N));
	rfwhip_light_count lc = {0, 1, 0, 0};
	ABI(rfwhip_set_lights(c, lc, nullptr, reinterpret_cast<const rfwhip_point_light *>(&s.pl), nullptr, nullptr));
	ABI(rfwhip_group_update(g));
	const rfw::Camera cam = camera();
	rfwhip_camera pod;
	std::memcpy(&pod, &cam, sizeof(pod));
	std::vector<float> linear(size_t(W) * H * 4);
	std::vector<uint8_t> bytes(size_t(W) * H * 4);
	ABI(rfwhip_group_render(g, &pod, RFWHIP_RESET));
	ABI(rfwhip_group_read_framebuffer(g, linear.data()));
	ABI(rfwhip_group_read_display(g, RFWHIP_DISPLAY_RGBA8, bytes.data()));
	rfwhip_group_destroy(g);
	if (int r = dump(out + "/abi.f32", linear.data(), linear.size() * sizeof(float)))
		return r;
	return dump(out + "/abi.rgba8", bytes.data(), bytes.size());
}

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".", out = argc > 2 ? argv[2] : ".";
	const char *tonemap = std::getenv("RFWHIP_DISPLAY") ? std::getenv("RFWHIP_DISPLAY") : "aces";
	SceneData s;
	void *h = dlopen((dir + "/HipRT.so").c_str(), RTLD_NOW);
	if (!h)
	{
		std::fprintf(stderr, "dlopen failed: %s\n", dlerror());
		return 2;
	}
	auto create = (CreateFn)dlsym(h, "createRenderContext");
	auto destroy = (DestroyFn)dlsym(h, "destroyRenderContext");
	auto read_display = (ReadFn)dlsym(h, "hiprtReadDisplay");
	if (!create || !destroy || !read_display)
		return 3;
	int rc = 0;
	try
	{
		rfw::RenderContext *ctx = create();
		if (int r = reference(s, tonemap, out))
			return r;
		GLuint tex = 0;
		ctx->init(&tex, W, H);
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
		std::vector<uint8_t> img(size_t(W) * H * 4);
		ctx->render_frame(camera(), rfw::Reset);
		if (read_display(ctx, img.data()) != 0)
			rc = 4;
		if (int r = dump(out + "/plugin.rgba8", img.data(), img.size()))
			rc = r;
		std::printf("size %u %u\n", W, H);
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
