// HipRT.cpp — the rfw::RenderContext plugin in front of the HIP rendercore: the drop-in for RFW/backends/.
//
// Built as "HipRT.so" (no lib prefix: rfw::system dlopens "<cwd>/<name>.so", RFW/system/src/rfw/system.cpp:119-121)
// and exports the two factory symbols of RFW/system/context/rfw/context/export.h:8-15.  Every virtual call forwards
// to one entry point of include/rfwhip.h; C status codes become std::runtime_error, which is how the reference's
// backends report failures across the plugin boundary (context.h:84-91, utils/logger.h:83-95).
//
// Devices: RFWHIP_DEVICES = "0-7" / "0,2,5" (default: RFWHIP_DEVICE or 0) — the plugin always sits on an rfwhip_group: one
// host thread (the reference's render loop, RFW/system/src/rfw/app.cpp:3-26) drives one context per device, every scene call
// is repeated per context, and the strips are gathered over xGMI (RCCL, or RFWHIP_TRANSPORT=peer) into device 0's image.
//
// Frames in flight: RFWHIP_FRAMES_IN_FLIGHT=n (1..4, default 1) — render_frame(k) enqueues frame k and its presentation and
// returns with frame k - n + 1 on the host (rfwhip_group_present_async / _wait): the devices never idle between frames; with 1
// it returns with frame k finished, like the reference's backends.
//
// Display stage: RFWHIP_DISPLAY=aces|none (unset by default: nothing changes) — render_frame presents the 8-bit display image of
// include/rfwhip.h (rfwhip_read_display: the reference's tone map with the camera's brightness / contrast, FXAA; "none": no tone
// curve) instead of the float image: rfwhip_group_present_display_async / _wait with frames in flight, a quarter of the bytes over
// PCIe, and the GL upload is GL_RGBA / GL_UNSIGNED_BYTE.  Leave it unset under rfw::system with toneMap = true: the system
// tone-maps again on top of whatever the backend delivers (system.cpp:682-711).  Headless hosts read the bytes with
// hiprtReadDisplay.
//
// Exposure: RFWHIP_EXPOSURE=auto|manual beside RFWHIP_DISPLAY (unset by default: nothing changes) sets display_exposure — with
// auto every presented display image is metered on the device behind the gather and shown with the adapted exposure (include/rfwhip.h,
// rfwhip_get_meter: one step per present, nothing read back, frames in flight stay in flight); RFWHIP_EXPOSURE_SPEED (optional) is
// display_exposure_speed.  A host reads the meter's record with hiprtGetExposure: with frames in flight it is the newest
// frame's, not the one render_frame handed out.
//
// Bloom: RFWHIP_BLOOM=1|0 beside RFWHIP_DISPLAY (unset by default: nothing changes) sets display_bloom — with 1 every presented
// display image gets the glow pyramid of include/rfwhip.h (rfwhip_bloom_image) in front of the tone map, on the device, behind the
// gather and the meter's step; the other display_bloom_* settings keep their defaults.
//
// Colour grading: RFWHIP_GRADE=1|0 beside RFWHIP_DISPLAY (unset by default: nothing changes) sets display_grade — with 1 every
// presented display image goes through the graded display kernel of include/rfwhip.h (rfwhip_set_display_lut).  Beside it:
// RFWHIP_GRADE_TEMPERATURE (display_wb_temperature, kelvin), RFWHIP_GRADE_SATURATION (display_grade_saturation),
// RFWHIP_GRADE_LUT=<path of a .cube file> (rfwhip_group_set_display_lut_cube) and RFWHIP_DITHER=1|0 (display_dither); a value the
// setting refuses, or a file that cannot be read, ends the constructor with the message.
//
// JPEG: hiprtReadJpeg hands a headless host the display image as a baseline JPEG encoded on the device (include/rfwhip.h,
// rfwhip_read_display_jpeg): a few hundred kilobytes instead of 4 bytes per pixel.  RFWHIP_JPEG_QUALITY (display_jpeg_quality,
// 1 .. 100), RFWHIP_JPEG_SUBSAMPLING (444 | 420) and RFWHIP_JPEG_RESTART (display_jpeg_restart) are optional; a value the setting
// refuses ends the constructor with the message.  Nothing is allocated or launched until hiprtReadJpeg is called.
//
// Sky: RFWHIP_SKY_HDR=<path of a Radiance .hdr file> loads a sky at construction (include/rfwhip.h, rfwhip_group_set_sky_hdr: every
// device decodes its own replica; the system's set_sky replaces it as usual), RFWHIP_SKY_TABLE=host|device sets sky_table — who
// builds the alias table of sky_sampling; the key is listed by get_settings() as well.  A file that cannot be read or decoded, or a
// value the setting refuses, ends the constructor with the message.
//
// Noise estimate: RFWHIP_NOISE=1 (unset by default: nothing changes) turns the setting noise_estimate on (include/rfwhip.h,
// rfwhip_get_noise); a host asks hiprtGetNoise when to stop converging.  It answers for the accumulator — with frames in flight,
// for the newest frame enqueued, not the one render_frame handed out.
//
// Material maps: RFWHIP_MATERIAL_MAPS=1 (unset by default: nothing changes) turns the setting material_maps on (include/rfwhip.h):
// the path tracer reads the alpha mask and the roughness / metallic maps the system's materials carry.  hiprtGetSetting reads a
// setting of the core back, the read-only ones included ("material_maps_on": do the next frame's shade waves run the map kernels?).
//
// Headless by default (RenderTarget::BUFFER, context.h:27-34): the GPU box has no OpenGL.  With
// -DRFWHIP_PLUGIN_WITH_GL (needs GLEW, i.e. the reference's own build environment) render_frame also uploads the
// float4 image into the GL texture handed to init(), the same way EmbreeRT presents (EmbreeRT/src/Context.cpp:289-297).
#ifdef RFWHIP_USE_RFW_HEADERS
#include <rfw/context/context.h>
#include <rfw/context/export.h>
#if __has_include(<rfw/context/blue_noise.h>)
#include <rfw/context/blue_noise.h> // createBlueNoiseBuffer(): the sampler table lives in the reference tree
#define RFWHIP_HAVE_BLUE_NOISE_TABLE 1
#endif
#else
#include "rfw/restated_context.h"
#endif
#include "rfwhip.h"

#ifdef RFWHIP_PLUGIN_WITH_GL
#include <GL/glew.h>
#endif

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace
{

[[noreturn]] void fail(const char *what)
{
	throw std::runtime_error(std::string("HipRT: ") + what + ": " + rfwhip_last_error());
}
#define HIPRT_CHECK(call)          \
	do                             \
	{                              \
		if ((call) != RFWHIP_OK)   \
			fail(#call);           \
	} while (0)

// The launcher's environment, one row per variable: a new RFWHIP_* variable that sets a setting is one more row here.  The rows are
// applied top to bottom at construction, and settings are order-dependent in the core: keep the order.  Two allowed values
// mean the plugin judges the value itself ("HipRT: <name> must be ..."); none, that it is passed through and the core judges it.
// A row without a key names a file that is read whole and handed to the core.
enum EnvFile
{
	NO_FILE,
	CUBE_FILE, // rfwhip_group_set_display_lut_cube
	HDR_FILE   // rfwhip_group_set_sky_hdr
};
struct EnvVar
{
	const char *name, *key = nullptr, *a = nullptr, *b = nullptr;
	EnvFile file = NO_FILE;
};
const EnvVar kEnv[] = {
	{"RFWHIP_DISPLAY", "display_tonemap", "aces", "none"}, // (and Context::m_Display)
	{"RFWHIP_EXPOSURE", "display_exposure", "auto", "manual"},
	{"RFWHIP_EXPOSURE_SPEED", "display_exposure_speed"},
	{"RFWHIP_BLOOM", "display_bloom", "0", "1"},
	{"RFWHIP_GRADE", "display_grade", "0", "1"},
	{"RFWHIP_GRADE_TEMPERATURE", "display_wb_temperature"},
	{"RFWHIP_GRADE_SATURATION", "display_grade_saturation"},
	{"RFWHIP_DITHER", "display_dither", "0", "1"},
	{"RFWHIP_GRADE_LUT", nullptr, nullptr, nullptr, CUBE_FILE},
	{"RFWHIP_JPEG_QUALITY", "display_jpeg_quality"},
	{"RFWHIP_JPEG_SUBSAMPLING", "display_jpeg_subsampling"},
	{"RFWHIP_JPEG_RESTART", "display_jpeg_restart"},
	{"RFWHIP_NOISE", "noise_estimate", "0", "1"},
	{"RFWHIP_MATERIAL_MAPS", "material_maps", "0", "1"},
	{"RFWHIP_SKY_TABLE", "sky_table"},
	{"RFWHIP_SKY_HDR", nullptr, nullptr, nullptr, HDR_FILE},
};

// the whole file at `path`, named by the variable `name`
std::string read_file(const char *name, const char *path)
{
	FILE *f = std::fopen(path, "rb");
	if (!f)
		throw std::runtime_error(std::string("HipRT: ") + name + ": cannot read " + path);
	std::string bytes;
	char buf[65536];
	for (size_t n; (n = std::fread(buf, 1, sizeof(buf), f)) > 0;)
		bytes.append(buf, n);
	std::fclose(f);
	return bytes;
}

class Context final : public rfw::RenderContext
{
  public:
	Context()
	{
		// the launcher's environment selects the devices: "0-7", "0,2,5", or a single RFWHIP_DEVICE
		std::vector<int> devices;
		if (const char *list = std::getenv("RFWHIP_DEVICES"))
			devices = parse_devices(list);
		if (devices.empty())
		{
			const char *dev = std::getenv("RFWHIP_DEVICE");
			devices.push_back(dev ? std::atoi(dev) : 0);
		}
		int transport = RFWHIP_TRANSPORT_AUTO;
		if (const char *t = std::getenv("RFWHIP_TRANSPORT"))
			transport = std::string(t) == "peer" ? RFWHIP_TRANSPORT_PEER : (std::string(t) == "rccl" ? RFWHIP_TRANSPORT_RCCL : RFWHIP_TRANSPORT_AUTO);
		HIPRT_CHECK(rfwhip_group_create(devices.data(), (int)devices.size(), transport, &m_Group));
		for (int i = 0; i < rfwhip_group_size(m_Group); i++)
			m_Cores.push_back(rfwhip_group_context(m_Group, i));
		if (const char *f = std::getenv("RFWHIP_FRAMES_IN_FLIGHT"))
			m_InFlight = std::max(1, std::min(RFWHIP_PRESENT_SLOTS, std::atoi(f)));
		for (const EnvVar &v : kEnv)
		{
			const char *value = std::getenv(v.name);
			if (!value)
				continue;
			if (v.a && std::strcmp(value, v.a) != 0 && std::strcmp(value, v.b) != 0)
				throw std::runtime_error(std::string("HipRT: ") + v.name + " must be \"" + v.a + "\" or \"" + v.b + "\"");
			if (v.key)
				HIPRT_CHECK(rfwhip_group_set_setting(m_Group, v.key, value));
			else if (v.file == CUBE_FILE)
			{
				const std::string text = read_file(v.name, value);
				HIPRT_CHECK(rfwhip_group_set_display_lut_cube(m_Group, text.data(), text.size()));
			}
			else
			{
				const std::string bytes = read_file(v.name, value);
				HIPRT_CHECK(rfwhip_group_set_sky_hdr(m_Group, bytes.data(), bytes.size(), 0));
			}
		}
		m_Display = std::getenv("RFWHIP_DISPLAY") != nullptr; // render_frame presents the display image
		const char *integ = std::getenv("RFWHIP_INTEGRATOR");
		HIPRT_CHECK(rfwhip_group_set_setting(m_Group, "integrator", integ ? integ : "pt"));
		if (m_InFlight >= RFWHIP_PRESENT_SLOTS) // four frames in flight need four sets of wave buffers (the default ring is three)
			HIPRT_CHECK(rfwhip_group_set_setting(m_Group, "ring", "4"));
#ifdef RFWHIP_HAVE_BLUE_NOISE_TABLE
		{
			// what CUDART does at init (CUDART/src/Context.cpp:43-46): primary rays then use blueNoiseSampler
			const std::vector<unsigned int> table = createBlueNoiseBuffer();
			for (rfwhip_context *c : m_Cores)
				HIPRT_CHECK(rfwhip_set_blue_noise(c, table.data(), table.size()));
			HIPRT_CHECK(rfwhip_group_set_setting(m_Group, "sampler", "bluenoise"));
		}
#endif
	}
	~Context() override
	{
		rfwhip_group_destroy(m_Group);
		m_Group = nullptr, m_Cores.clear();
	}

	static std::vector<int> parse_devices(const std::string &list)
	{
		std::vector<int> out;
		size_t pos = 0;
		while (pos < list.size())
		{
			size_t end = list.find(',', pos);
			if (end == std::string::npos)
				end = list.size();
			const std::string item = list.substr(pos, end - pos);
			const size_t dash = item.find('-');
			if (!item.empty())
			{
				const int a = std::atoi(item.c_str()), b = dash == std::string::npos ? a : std::atoi(item.c_str() + dash + 1);
				for (int d = a; d <= b && out.size() < 64; d++)
					out.push_back(d);
			}
			pos = end + 1;
		}
		return out;
	}

	[[nodiscard]] std::vector<rfw::RenderTarget> get_supported_targets() const override
	{
#ifdef RFWHIP_PLUGIN_WITH_GL
		return {rfw::RenderTarget::OPENGL_TEXTURE, rfw::RenderTarget::BUFFER};
#else
		return {rfw::RenderTarget::BUFFER};
#endif
	}

	void init(std::shared_ptr<rfw::utils::window> &) override
	{
		throw std::runtime_error("HipRT: window targets are not supported.");
	}

	void init(GLuint *glTextureID, uint width, uint height) override
	{
		m_Target = glTextureID ? *glTextureID : 0;
		m_Width = width, m_Height = height;
		HIPRT_CHECK(rfwhip_group_init(m_Group, width, height));
		// a resize frees the pinned host images of the frames in flight: the window of frames starts over
		m_Frame = 0, m_Latest = nullptr, m_LatestDisplay = nullptr;
		m_Host.assign(size_t(width) * height * 4, 0.0f);
		m_HostDisplay.assign(m_Display ? size_t(width) * height * 4 : 0, 0);
	}

	void cleanup() override
	{
		if (m_Group && !m_Cleaned) // idempotent: called from system::unload and again from destroyRenderContext
		{
			HIPRT_CHECK(rfwhip_group_wait(m_Group));
			for (rfwhip_context *c : m_Cores)
				HIPRT_CHECK(rfwhip_cleanup(c));
			m_Cleaned = true;
		}
	}

	void render_frame(const rfw::Camera &camera, rfw::RenderStatus status) override
	{
		static_assert(sizeof(rfw::Camera) >= sizeof(rfwhip_camera), "camera layout");
		rfwhip_camera cam;
		std::memcpy(&cam, &camera, sizeof(cam)); // position .. pixelCount are the first 60 bytes (camera.h:27-37)
		HIPRT_CHECK(rfwhip_group_render(m_Group, &cam, status == rfw::Reset ? RFWHIP_RESET : RFWHIP_CONVERGE));
		const float *image = nullptr;
		const void *display = nullptr;
		if (m_InFlight >= 2)
		{
			// frame k and its way to the host are enqueued; what is handed out is frame k - (n - 1) (the first n - 1 calls wait
			// for frame 0, their own oldest)
			const int n = m_InFlight, slot = (int)(m_Frame % (unsigned)n);
			const unsigned long long oldest = m_Frame >= (unsigned)(n - 1) ? m_Frame - (unsigned)(n - 1) : 0;
			if (m_Display)
			{
				HIPRT_CHECK(rfwhip_group_present_display_async(m_Group, slot, RFWHIP_DISPLAY_RGBA8));
				HIPRT_CHECK(rfwhip_group_present_display_wait(m_Group, (int)(oldest % (unsigned)n), &display, nullptr));
			}
			else
			{
				HIPRT_CHECK(rfwhip_group_present_async(m_Group, slot));
				HIPRT_CHECK(rfwhip_group_present_wait(m_Group, (int)(oldest % (unsigned)n), &image));
			}
		}
		else
			HIPRT_CHECK(rfwhip_group_wait(m_Group)); // the reference's render_frame returns with the frame finished
		m_Latest = image, m_LatestDisplay = static_cast<const uint8_t *>(display);
		m_Frame++;
#ifdef RFWHIP_PLUGIN_WITH_GL
		if (m_Target && m_Display)
		{
			if (!display)
			{
				HIPRT_CHECK(rfwhip_group_read_display(m_Group, RFWHIP_DISPLAY_RGBA8, m_HostDisplay.data()));
				display = m_HostDisplay.data();
			}
			glBindTexture(GL_TEXTURE_2D, m_Target);
			glTexSubImage2D(GL_TEXTURE_2D, 0, 0, 0, m_Width, m_Height, GL_RGBA, GL_UNSIGNED_BYTE, display);
		}
		else if (m_Target)
		{
			if (!image)
			{
				HIPRT_CHECK(rfwhip_group_read_framebuffer(m_Group, m_Host.data()));
				image = m_Host.data();
			}
			glBindTexture(GL_TEXTURE_2D, m_Target);
			glTexSubImage2D(GL_TEXTURE_2D, 0, 0, 0, m_Width, m_Height, GL_RGBA, GL_FLOAT, image);
		}
#endif
	}

	// headless read-back: the frame render_frame last handed out (frames in flight: frame k - 1, already on the host)
	int read(float *rgba)
	{
		if (m_Latest)
		{
			std::memcpy(rgba, m_Latest, size_t(m_Width) * m_Height * 4 * sizeof(float));
			return RFWHIP_OK;
		}
		return rfwhip_group_read_framebuffer(m_Group, rgba);
	}

	// ... and the display image (RGBA8) of that frame: with RFWHIP_DISPLAY and frames in flight the bytes render_frame received,
	// else the display stage of the newest frame, read now
	int read_display(uint8_t *rgba8)
	{
		if (m_LatestDisplay)
		{
			std::memcpy(rgba8, m_LatestDisplay, size_t(m_Width) * m_Height * 4);
			return RFWHIP_OK;
		}
		return rfwhip_group_read_display(m_Group, RFWHIP_DISPLAY_RGBA8, rgba8);
	}

	// ... and the display image of the newest frame as a baseline JPEG, encoded on the device and read now (with frames in flight
	// that is the newest frame enqueued, not the one render_frame handed out); bound: the capacity that always suffices
	int read_jpeg(void *out, size_t cap, size_t *bytes) { return rfwhip_group_read_display_jpeg(m_Group, out, cap, bytes); }
	int jpeg_bound(size_t *bytes) { return rfwhip_display_jpeg_bound(m_Cores[0], bytes); }

	// the noise of the accumulated image (RFWHIP_NOISE=1; else RFWHIP_ERR_STATE)
	int get_noise(rfwhip_noise_stats *stats) { return rfwhip_group_get_noise(m_Group, stats); }
	// the exposure meter's record (RFWHIP_EXPOSURE=auto; else exposure 1 and no steps)
	int get_exposure(rfwhip_meter_stats *stats) { return rfwhip_group_get_meter(m_Group, stats); }

	void set_materials(const std::vector<rfw::DeviceMaterial> &materials,
					   const std::vector<rfw::MaterialTexIds> &texDescriptors) override
	{
		for (rfwhip_context *c : m_Cores)
			HIPRT_CHECK(rfwhip_set_materials(c, reinterpret_cast<const rfwhip_material *>(materials.data()),
										 reinterpret_cast<const rfwhip_material_tex_ids *>(texDescriptors.data()),
										 materials.size()));
	}

	void set_textures(const std::vector<rfw::TextureData> &textures) override
	{
		for (rfwhip_context *c : m_Cores)
			HIPRT_CHECK(rfwhip_set_textures(c, reinterpret_cast<const rfwhip_texture *>(textures.data()), textures.size()));
	}

	void set_mesh(size_t index, const rfw::Mesh &mesh) override
	{
		for (rfwhip_context *c : m_Cores)
			HIPRT_CHECK(rfwhip_set_mesh(c, index, reinterpret_cast<const rfwhip_mesh *>(&mesh)));
	}

	void set_instance(size_t i, size_t meshIdx, const glm::mat4 &transform, const glm::mat3 &inverse_transform) override
	{
		for (rfwhip_context *c : m_Cores)
			HIPRT_CHECK(rfwhip_set_instance(c, i, meshIdx, reinterpret_cast<const float *>(&transform),
										reinterpret_cast<const float *>(&inverse_transform)));
	}

	void set_sky(const std::vector<glm::vec3> &pixels, size_t width, size_t height) override
	{
		for (rfwhip_context *c : m_Cores)
			HIPRT_CHECK(rfwhip_set_sky(c, reinterpret_cast<const float *>(pixels.data()), width, height));
	}

	void set_lights(rfw::LightCount lightCount, const rfw::DeviceAreaLight *areaLights,
					const rfw::DevicePointLight *pointLights, const rfw::DeviceSpotLight *spotLights,
					const rfw::DeviceDirectionalLight *directionalLights) override
	{
		rfwhip_light_count n;
		std::memcpy(&n, &lightCount, sizeof(n));
		for (rfwhip_context *c : m_Cores)
			HIPRT_CHECK(rfwhip_set_lights(c, n, reinterpret_cast<const rfwhip_area_light *>(areaLights),
									  reinterpret_cast<const rfwhip_point_light *>(pointLights),
									  reinterpret_cast<const rfwhip_spot_light *>(spotLights),
									  reinterpret_cast<const rfwhip_directional_light *>(directionalLights)));
	}

	void get_probe_results(unsigned int *instanceIndex, unsigned int *primitiveIndex, float *distance) const override
	{
		// the probe pixel belongs to one rank's strips; the others report nothing for it.  (The probe record is read back by a
		// wait; with frames in flight nothing else waits.)
		if (m_InFlight >= 2)
			HIPRT_CHECK(rfwhip_group_wait(m_Group));
		unsigned int inst = 0, prim = 0;
		float dist = 0.0f;
		// only the rank that owns the probe pixel's 8-row strip has a record for it (every context keeps its last valid one:
		// asking the others would hand back the hit of wherever the probe was before)
		{
			const int owner = rfwhip_row_owner((int)m_ProbeY, (int)m_Cores.size()); // rfwhip.h: serpentine strip ownership
			HIPRT_CHECK(rfwhip_get_probe_results(m_Cores[(size_t)owner], &inst, &prim, &dist));
		}
		if (instanceIndex)
			*instanceIndex = inst;
		if (primitiveIndex)
			*primitiveIndex = prim;
		if (distance)
			*distance = dist;
	}

	rfw::AvailableRenderSettings get_settings() const override
	{
		rfw::AvailableRenderSettings s;
		s.settingKeys = {"integrator", "jitter", "spp", "max_depth", "DENOISE", "DENOISE_TEMPORAL", "sky_sampling", "DENOISE_MOTION", "sky_table"};
		s.settingValues = {{"pt", "parity"}, {"xor128", "center"}, {"1", "2", "4", "8", "16"}, {"0", "1", "2", "3", "4"}, {"0", "1"},
						   {"0", "1"}, {"0", "1"}, {"0", "1"}, {"host", "device"}};
		return s;
	}

	void set_setting(const rfw::RenderSetting &setting) override
	{
		// the reference's OptiX 6 key (OptiXContext.cpp:812-822): the denoised image is what render_frame hands out
		// ... and its temporal stage (the history follows the frames render_frame presents), with or without motion
		const char *key = setting.name == "DENOISE"			 ? "denoise"
						  : setting.name == "DENOISE_TEMPORAL" ? "denoise_temporal"
						  : setting.name == "DENOISE_MOTION"   ? "denoise_motion"
															   : setting.name.c_str();
		HIPRT_CHECK(rfwhip_group_set_setting(m_Group, key, setting.value.c_str()));
	}

	void update() override { HIPRT_CHECK(rfwhip_group_update(m_Group)); }

	void set_probe_index(glm::uvec2 probePos) override
	{
		m_ProbeY = probePos.y;
		for (rfwhip_context *c : m_Cores)
			HIPRT_CHECK(rfwhip_set_probe_index(c, probePos.x, probePos.y));
	}

	rfw::RenderStats get_stats() const override
	{
		// ray counts add up over the ranks; the times are the slowest rank's
		rfwhip_render_stats st;
		if (m_InFlight >= 2)
			HIPRT_CHECK(rfwhip_group_wait(m_Group)); // (the stats are resolved by a wait; with frames in flight nothing else waits)
		HIPRT_CHECK(rfwhip_get_stats(m_Cores[0], &st));
		for (size_t k = 1; k < m_Cores.size(); k++)
		{
			rfwhip_render_stats r;
			HIPRT_CHECK(rfwhip_get_stats(m_Cores[k], &r));
			st.primaryCount += r.primaryCount, st.secondaryCount += r.secondaryCount, st.deepCount += r.deepCount, st.shadowCount += r.shadowCount;
			st.primaryTime = std::max(st.primaryTime, r.primaryTime), st.secondaryTime = std::max(st.secondaryTime, r.secondaryTime);
			st.deepTime = std::max(st.deepTime, r.deepTime), st.shadowTime = std::max(st.shadowTime, r.shadowTime);
			st.shadeTime = std::max(st.shadeTime, r.shadeTime), st.finalizeTime = std::max(st.finalizeTime, r.finalizeTime);
			st.renderTime = std::max(st.renderTime, r.renderTime), st.animationTime = std::max(st.animationTime, r.animationTime);
		}
		rfw::RenderStats out;
		std::memcpy(&out, &st, sizeof(out));
		return out;
	}

	int get_setting(const char *key, char *out, size_t cap) const { return rfwhip_get_setting(m_Cores[0], key, out, cap); }

	rfwhip_group *group() const { return m_Group; }

  private:
	rfwhip_group *m_Group = nullptr;
	std::vector<rfwhip_context *> m_Cores;
	bool m_Cleaned = false;
	int m_InFlight = 1;
	unsigned long long m_Frame = 0;
	unsigned m_ProbeY = 0; // row of the probe pixel: decides which rank's record get_probe_results reads
	const float *m_Latest = nullptr;
	bool m_Display = false; // RFWHIP_DISPLAY: render_frame presents the display image
	const uint8_t *m_LatestDisplay = nullptr;
	std::vector<uint8_t> m_HostDisplay;
	GLuint m_Target = 0;
	uint m_Width = 0, m_Height = 0;
	std::vector<float> m_Host;
};

} // namespace

#define HIPRT_EXPORT extern "C" __attribute__((visibility("default")))

// export.h:14-15
HIPRT_EXPORT rfw::RenderContext *createRenderContext() { return new Context(); }
HIPRT_EXPORT void destroyRenderContext(rfw::RenderContext *ptr)
{
	ptr->cleanup(); // every reference backend does this too (EmbreeRT/src/Context.cpp:30)
	delete ptr;
}

// Headless hosts (no GL texture to look at) read the BUFFER target through this extra symbol.
HIPRT_EXPORT int hiprtReadFramebuffer(rfw::RenderContext *ptr, float *rgba)
{
	return static_cast<Context *>(ptr)->read(rgba);
}
// ... and the presentable image: width * height * 4 bytes, R first (the display stage, include/rfwhip.h rfwhip_read_display)
HIPRT_EXPORT int hiprtReadDisplay(rfw::RenderContext *ptr, uint8_t *rgba8)
{
	return static_cast<Context *>(ptr)->read_display(rgba8);
}
// ... and the same image as a baseline JPEG (include/rfwhip.h rfwhip_read_display_jpeg): at most `cap` bytes into `out`, *bytes = the
// stream's length (also when cap is too small: RFWHIP_ERR_INVALID_ARGUMENT, nothing written); hiprtJpegBound: the cap that always suffices
HIPRT_EXPORT int hiprtReadJpeg(rfw::RenderContext *ptr, void *out, size_t cap, size_t *bytes)
{
	return static_cast<Context *>(ptr)->read_jpeg(out, cap, bytes);
}
HIPRT_EXPORT int hiprtJpegBound(rfw::RenderContext *ptr, size_t *bytes)
{
	return static_cast<Context *>(ptr)->jpeg_bound(bytes);
}
// ... and how noisy the accumulated image still is (the noise estimate, include/rfwhip.h rfwhip_get_noise): 0, or an rfwhip_status
// (rfwhip_last_error has the text) — without RFWHIP_NOISE=1, or before the second sample
HIPRT_EXPORT int hiprtGetNoise(rfw::RenderContext *ptr, rfwhip_noise_stats *stats)
{
	return static_cast<Context *>(ptr)->get_noise(stats);
}
// ... and how the display image is exposed (the exposure meter, include/rfwhip.h rfwhip_get_meter): the record of the newest frame
// presented — exposure, its log2, the target, the metered luminance, valid / excluded pixels and the steps taken
HIPRT_EXPORT int hiprtGetExposure(rfw::RenderContext *ptr, rfwhip_meter_stats *stats)
{
	return static_cast<Context *>(ptr)->get_exposure(stats);
}
// ... and a setting of the core as text (include/rfwhip.h rfwhip_get_setting; every device holds the same): 0, or an rfwhip_status
HIPRT_EXPORT int hiprtGetSetting(rfw::RenderContext *ptr, const char *key, char *out, size_t cap)
{
	return static_cast<Context *>(ptr)->get_setting(key, out, cap);
}
