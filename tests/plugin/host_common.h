// host_common.h — what the stand-ins for rfw::system's side of the plugin boundary (tests/plugin/*_host.cpp) share: how "HipRT.so"
// is opened and closed, the scene every host but plugin_host.cpp renders, and that scene's way through the virtual interface and
// through the C ABI.  A new host holds its header comment (the protocol its pytest file relies on), its environment variables, its
// frame loop and what it prints and writes; tests/plugin_hosts.py compiles and starts it.
//
// Exit statuses: 2 dlopen failed (dlerror() on stderr), 3 a symbol is missing, 5 an exception crossed the boundary ("exception:
// <what>" on stderr; a value the plugin's constructor refuses ends here), 6 a C ABI call failed (ABI), 7 a file could not be written
// (dump).  A host's own: 4 a hiprt* read failed.
#pragma once
#include "rfw/restated_context.h"
#include "rfwhip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <initializer_list>
#include <string>
#include <vector>

typedef rfw::RenderContext *(*CreateFn)();
typedef void (*DestroyFn)(rfw::RenderContext *);
typedef int (*ReadFn)(rfw::RenderContext *, float *);		   // hiprtReadFramebuffer
typedef int (*ReadDisplayFn)(rfw::RenderContext *, uint8_t *); // hiprtReadDisplay

static const uint W = 96, H = 64;

// HipRT.so of the directory `dir`: the two factory symbols (export.h:14-15) and the hiprt* symbols a host names, in its order
struct Plugin
{
	void *lib = nullptr;
	CreateFn create = nullptr;
	DestroyFn destroy = nullptr;
	std::vector<void *> sym;
	int open(const std::string &dir, std::initializer_list<const char *> names)
	{
		lib = dlopen((dir + "/HipRT.so").c_str(), RTLD_NOW);
		if (!lib)
		{
			std::fprintf(stderr, "dlopen failed: %s\n", dlerror());
			return 2;
		}
		create = (CreateFn)dlsym(lib, "createRenderContext");
		destroy = (DestroyFn)dlsym(lib, "destroyRenderContext");
		bool all = create && destroy;
		for (const char *name : names)
		{
			sym.push_back(dlsym(lib, name));
			all = all && sym.back();
		}
		return all ? 0 : 3;
	}
};

// The life of one context: create, body(ctx, rc), cleanup (system::unload calls it, then destroy calls it again), destroy, dlclose.
// The body leaves a failure that does not stop it in rc (4, 7) and returns 0; what it returns otherwise ends the program with that
// status at once.  Returns the exit status.
template <class Body> static inline int drive(const Plugin &p, Body body)
{
	int rc = 0;
	try
	{
		rfw::RenderContext *ctx = p.create();
		if (int r = body(ctx, rc))
			return r;
		ctx->cleanup();
		p.destroy(ctx);
	}
	catch (const std::exception &e)
	{
		std::fprintf(stderr, "exception: %s\n", e.what());
		rc = 5;
	}
	dlclose(p.lib);
	return rc;
}

// the quad of plugin_host.cpp facing the camera at z = 4, a second quad behind it (depth and normal edges for the filters) with a
// material of its own, a point light at the origin, and a sky of one colour: {0.25, 0.5, 0.75}, or {2, 4, 8} — far above display
// white: it shows left and right of the back quad and bleeds over its edges
struct SceneData
{
	rfw::DeviceMaterial mat[2];
	rfw::MaterialTexIds ids[2];
	float verts[8][4] = {{-1, -1, 4, 1}, {1, -1, 4, 1}, {1, 1, 4, 1}, {-1, 1, 4, 1},
						 {-3, -3, 7, 1}, {3, -3, 6, 1}, {3, 3, 6, 1}, {-3, 3, 7, 1}};
	unsigned idx[4][3] = {{0, 2, 1}, {0, 3, 2}, {4, 6, 5}, {4, 7, 6}};
	rfw::Triangle tris[4];
	std::vector<glm::vec3> sky;
	rfw::DevicePointLight pl;
	rfw::Mesh mesh;
	explicit SceneData(glm::vec3 sky_colour) : sky(8 * 4, sky_colour)
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

static inline rfw::Camera camera()
{
	rfw::Camera cam;
	std::memset(&cam, 0, sizeof(cam));
	cam.direction.z = 1.0f, cam.focalDistance = 5.0f, cam.FOV = 40.0f, cam.aspectRatio = float(W) / H, cam.clampValue = 10.0f;
	cam.pixelCount = glm::ivec2{int(W), int(H)};
	cam.brightness = 0.05f, cam.contrast = 1.0f; // Camera.cpp:8-9 (the display stage reads them)
	return cam;
}

// ... and what the C ABI takes: position .. pixelCount, the first 60 bytes (camera.h:27-37)
static inline rfwhip_camera pod(const rfw::Camera &cam)
{
	rfwhip_camera c;
	std::memcpy(&c, &cam, sizeof(c));
	return c;
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

static inline int dump(const std::string &path, const void *data, size_t bytes)
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

// the scene through the virtual interface, in system::synchronize's order; settings(): what a host sets between init and the scene
template <class Settings> static inline void upload(rfw::RenderContext *ctx, const SceneData &s, Settings settings)
{
	GLuint tex = 0;
	ctx->init(&tex, W, H);
	settings();
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
}
static inline void upload(rfw::RenderContext *ctx, const SceneData &s)
{
	upload(ctx, s, [] {});
}

// the same scene through the C ABI, after the host's init and settings: into one context, or into a group of one
static inline int scene_abi(rfwhip_context *c, const SceneData &s)
{
	ABI(rfwhip_set_sky(c, reinterpret_cast<const float *>(s.sky.data()), 8, 4));
	ABI(rfwhip_set_textures(c, nullptr, 0));
	ABI(rfwhip_set_materials(c, reinterpret_cast<const rfwhip_material *>(s.mat), reinterpret_cast<const rfwhip_material_tex_ids *>(s.ids), 2));
	ABI(rfwhip_set_mesh(c, 0, reinterpret_cast<const rfwhip_mesh *>(&s.mesh)));
	const float M[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, N[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
	ABI(rfwhip_set_instance(c, 0, 0, M, N));
	rfwhip_light_count lc = {0, 1, 0, 0};
	ABI(rfwhip_set_lights(c, lc, nullptr, reinterpret_cast<const rfwhip_point_light *>(&s.pl), nullptr, nullptr));
	return 0;
}
static inline int upload_abi(rfwhip_context *c, const SceneData &s)
{
	if (int r = scene_abi(c, s))
		return r;
	ABI(rfwhip_update(c));
	return 0;
}
static inline int upload_abi(rfwhip_group *g, const SceneData &s)
{
	if (int r = scene_abi(rfwhip_group_context(g, 0), s))
		return r;
	ABI(rfwhip_group_update(g));
	return 0;
}

// a group of one context on device 0, initialised at W x H with the path tracer: where every host's reference group starts
static inline int reference_group(rfwhip_group **g)
{
	const int device = 0;
	ABI(rfwhip_group_create(&device, 1, RFWHIP_TRANSPORT_AUTO, g));
	ABI(rfwhip_group_init(*g, W, H));
	ABI(rfwhip_group_set_setting(*g, "integrator", "pt"));
	return 0;
}
