// animation_san_main.cpp — the validator and the work items of csrc/animation.h over exactly-sized heap arrays, for the host
// sanitizers (tests/test_animation.py compiles this with -fsanitize=address,undefined and runs it in a child process).  It includes
// animation.h alone.  Per file of the command line (nine 64-bit counts — nodes, weights, skins, joints, CALLS, animations, channels,
// times, values — the tables in that order with 16 floats of inverse bind per joint in the fifth place, then (animation, time)
// pairs) it prints "<file> <validator's code> <message>", and for an accepted rig evaluates every call serially.  Last line: "done".
#include "animation.h"

#include <stdlib.h>

#include <string>

template <typename T> static T *exact(size_t n) // n elements and not a byte more, so that an overrun is the sanitizer's to see
{
	return (T *)malloc(n ? n * sizeof(T) : 1);
}

static bool run(const char *path)
{
	FILE *f = fopen(path, "rb");
	if (!f)
		return false;
	uint64_t c[9];
	if (fread(c, 8, 9, f) != 9)
		return fclose(f), false;
	const size_t calls = c[4];
	rtk::RigNode *nodes = exact<rtk::RigNode>(c[0]);
	float *weights = exact<float>(c[1]);
	rtk::RigSkin *skins = exact<rtk::RigSkin>(c[2]);
	uint32_t *joints = exact<uint32_t>(c[3]);
	float *ibm = exact<float>(16 * c[3]);
	rtk::RigAnim *anims = exact<rtk::RigAnim>(c[5]);
	rtk::RigChannel *channels = exact<rtk::RigChannel>(c[6]);
	float *times = exact<float>(c[7]), *values = exact<float>(c[8]);
	rtk::RigCall *list = exact<rtk::RigCall>(calls);
	bool ok = fread(nodes, sizeof(rtk::RigNode), c[0], f) == c[0] && fread(weights, 4, c[1], f) == c[1] && fread(skins, sizeof(rtk::RigSkin), c[2], f) == c[2] &&
			  fread(joints, 4, c[3], f) == c[3] && fread(ibm, 64, c[3], f) == c[3] && fread(anims, sizeof(rtk::RigAnim), c[5], f) == c[5] &&
			  fread(channels, sizeof(rtk::RigChannel), c[6], f) == c[6] && fread(times, 4, c[7], f) == c[7] && fread(values, 4, c[8], f) == c[8];
	for (size_t i = 0; ok && i < calls; i++)
	{
		list[i].rig = 0;
		ok = fread(&list[i].animation, 4, 1, f) == 1 && fread(&list[i].time, 4, 1, f) == 1;
	}
	fclose(f);
	if (ok)
	{
		rtk::RigSource src = {nodes, (size_t)c[0], weights, (size_t)c[1], skins, (size_t)c[2], joints, ibm, (size_t)c[3], anims, (size_t)c[5],
							  channels, (size_t)c[6], times, (size_t)c[7], values, (size_t)c[8]};
		rtk::RigPlan plan;
		const int rc = rtk::rig_validate(src, plan);
		printf("%s %d %s\n", path, rc, plan.msg);
		if (!rc)
		{
			const size_t n = c[0], items = plan.item_skin.size();
			rtk::RigView v;
			memset(&v, 0, sizeof(v));
			v.nodes = nodes, v.base_weights = weights, v.skins = skins, v.joints = joints, v.ibm = ibm, v.anims = anims, v.channels = channels;
			v.times = times, v.values = values;
			uint32_t *order = exact<uint32_t>(n), *level = exact<uint32_t>(plan.level_first.size()), *iskin = exact<uint32_t>(items), *ijoint = exact<uint32_t>(items);
			memcpy(order, plan.order.data(), n * 4), memcpy(level, plan.level_first.data(), plan.level_first.size() * 4);
			if (items)
				memcpy(iskin, plan.item_skin.data(), items * 4), memcpy(ijoint, plan.item_joint.data(), items * 4);
			v.order = order, v.level_first = level, v.item_skin = iskin, v.item_joint = ijoint;
			v.trs = exact<float>(rtk::RIG_TRS * n), v.weights = exact<float>(c[1]), v.world = exact<float>(16 * n), v.local = exact<float>(16 * n);
			v.inv = exact<float>(16 * c[2]), v.joint_mats = exact<float>(16 * items), v.flags = exact<uint32_t>(c[6] + c[2]);
			v.status = exact<rtk::RigStatus>(1);
			memset(v.status, 0, sizeof(rtk::RigStatus));
			v.node_count = (uint32_t)n, v.weight_count = (uint32_t)c[1], v.skin_count = (uint32_t)c[2], v.item_count = (uint32_t)items;
			v.anim_count = (uint32_t)c[5], v.channel_count = (uint32_t)c[6], v.levels = plan.levels;
			for (size_t i = 0; i < calls; i++)
				if (list[i].animation == rtk::RIG_BASE_POSE || list[i].animation < v.anim_count) // (what rfwhip_animate lets through)
					rtk::rig_host_evaluate(&v, list + i, 1);
			ok = v.status->serial == calls;
			free(order), free(level), free(iskin), free(ijoint), free(v.trs), free(v.weights), free(v.world), free(v.local), free(v.inv);
			free(v.joint_mats), free(v.flags), free(v.status);
		}
	}
	free(nodes), free(weights), free(skins), free(joints), free(ibm), free(anims), free(channels), free(times), free(values), free(list);
	return ok;
}

int main(int argc, char **argv)
{
	for (int i = 1; i < argc; i++)
		if (!run(argv[i]))
		{
			fprintf(stderr, "%s: unreadable, or an evaluation went missing\n", argv[i]);
			return 1;
		}
	printf("done\n");
	return 0;
}
