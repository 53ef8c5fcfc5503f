// jpeg_host.cpp — the JPEG of the presented frame through the plugin boundary: dlopen "HipRT.so" with RFWHIP_DISPLAY and the
// RFWHIP_JPEG_* variables the test sets in the environment, drive the rfw::RenderContext through its virtual interface for one frame
// and write what hiprtReadDisplay returns to <out>/plugin.rgba8 and what hiprtReadJpeg returns to <out>/plugin.jpg.
// tests/test_jpeg_plugin_gpu.py encodes plugin.rgba8 with the numpy model under the same settings and asks for equal bytes.  A value
// the plugin refuses ends the program (exit status 5, the message on stderr) before anything renders.  A second hiprtReadJpeg with
// a cap one byte short must fail, name the length and leave its buffer alone (exit status 8 otherwise).  Compiled by the test
// against the restated interface header and librfwhip.so.
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
typedef int (*JpegFn)(rfw::RenderContext *, void *, size_t, size_t *);
typedef int (*BoundFn)(rfw::RenderContext *, size_t *);

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

int main(int argc, char **argv)
{
	const std::string dir = argc > 1 ? argv[1] : ".", out = argc > 2 ? argv[2] : ".";
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
	auto read_jpeg = (JpegFn)dlsym(h, "hiprtReadJpeg");
	auto jpeg_bound = (BoundFn)dlsym(h, "hiprtJpegBound");
	if (!create || !destroy || !read_display || !read_jpeg || !jpeg_bound)
		return 3;
	int rc = 0;
	try
	{
		rfw::RenderContext *ctx = create();
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
		size_t bound = 0, bytes = 0, needed = 0;
		if (jpeg_bound(ctx, &bound) != 0)
			rc = 4;
		std::vector<uint8_t> jpg(bound), small(bound, 0xA5);
		if (read_jpeg(ctx, jpg.data(), jpg.size(), &bytes) != 0 || bytes > bound)
			rc = 4;
		else if (int r = dump(out + "/plugin.jpg", jpg.data(), bytes))
			rc = r;
		if (!rc && (read_jpeg(ctx, small.data(), bytes - 1, &needed) == 0 || needed != bytes || small[0] != 0xA5 || small[bytes - 1] != 0xA5))
			rc = 8;
		std::printf("size %u %u bound %zu bytes %zu\n", W, H, bound, bytes);
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
