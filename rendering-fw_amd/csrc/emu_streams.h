// emu_streams.h — deferred streams for the host-emulation build of the tests (-DRFWHIP_HOST_EMULATION -DRFWHIP_EMU_STREAMS=1,
// tests/_emu/librfwhip_emu_streams.so only; the product and the default emulation library never include this).
//
// In the default emulation build every "stream" is immediate: each launch runs when the host issues it, so a missing
// stream wait cannot change an image.  Here every device operation (kernel launch, copy, fill, event record) becomes a
// closure in the FIFO of its stream, and nothing runs until the host reaches a sync point (stream / event sync, a read
// back to the host, a free, a stream's destruction).  A sync point runs only what it needs: the target, its FIFO
// predecessors and, through the wait markers of stream_wait, the operations the waits name, transitively.  Which ready
// closure runs next is the policy's choice:
//   INORDER  the smallest enqueue number first (the order the host issued them: the immediate build's order)
//   LATE     the largest first: independent work is delayed as long as the dependencies allow
//   RANDOM   a seeded uniform choice among the ready closures
//   EAGER    latest first as well, but over everything enqueued on any stream, needed or not: a device runs independent work as
//            soon as it can, so an operation that overwrites what an earlier one still reads (a missing write-after-read wait)
//            runs ahead of that reader, which a sync point that runs only what it needs never does
// The model is HIP's and no stronger: streams are non-blocking (the null stream orders nothing with the others), a wait
// marker holds the event's record as it stood when the wait was enqueued (a re-record does not move it), a wait on an
// event that was never recorded is a no-op, and a free synchronises the device (hipFree does).
//
// One host thread drives the library (the group front end is single-threaded as well); a launch issued from inside a
// running closure (launch_shadow_packets -> launch_connect) runs at once, as part of that closure.
#pragma once
#if defined(RFWHIP_HOST_EMULATION) && defined(RFWHIP_EMU_STREAMS) && RFWHIP_EMU_STREAMS

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <deque>
#include <functional>
#include <memory>
#include <vector>

namespace emu_streams
{
enum Policy
{
	INORDER = 0,
	LATE = 1,
	RANDOM = 2,
	EAGER = 3
};

struct Op
{
	uint64_t seq = 0;
	std::function<void()> fn; // empty: a wait marker
	int wait_stream = -1;	  // (marker) the stream and position the event's record named when the wait was enqueued
	uint64_t wait_pos = 0;
};
struct Stream
{
	std::deque<Op> q;			// operations not run yet, in FIFO order
	uint64_t enq = 0, done = 0; // operations enqueued / run so far (positions are counts of operations)
};
struct Event
{
	int stream = -1; // never recorded: waits and syncs on it are no-ops
	uint64_t pos = 0, gen = 0;
	std::chrono::steady_clock::time_point t{};
	bool timed = false;
};
struct State
{
	std::vector<std::unique_ptr<Stream>> streams; // [0] is the null stream; a destroyed stream keeps its entry (markers name it)
	uint64_t seq = 0;
	int policy = INORDER;
	uint64_t rng = 0x9E3779B97F4A7C15ull;
	bool running = false;
	unsigned long long ran = 0, out_of_order = 0;
	unsigned long long shadow_packet_launches = 0; // launch_shadow_packets calls (the emulation runs them as plain connection waves)
	State() { streams.emplace_back(new Stream()); }
};
inline State &state()
{
	static State s;
	return s;
}
inline Stream &stream_of(void *s) { return *state().streams[(size_t)(uintptr_t)s]; }
inline bool deferring() { return !state().running; }

[[noreturn]] inline void fatal(const char *what)
{
	fprintf(stderr, "emu_streams: %s\n", what);
	abort();
}

inline void *stream_create()
{
	State &S = state();
	S.streams.emplace_back(new Stream());
	return (void *)(uintptr_t)(S.streams.size() - 1);
}

inline void enqueue(void *s, std::function<void()> fn)
{
	State &S = state();
	if (S.running) // (a launch from inside a running closure is part of it)
	{
		fn();
		return;
	}
	Stream &q = stream_of(s);
	Op op;
	op.seq = S.seq++, op.fn = std::move(fn);
	q.q.push_back(std::move(op));
	q.enq++;
}

inline void run_op(Stream &q)
{
	State &S = state();
	Op op = std::move(q.q.front());
	q.q.pop_front();
	if (op.fn)
	{
		S.running = true;
		op.fn();
		S.running = false;
		S.ran++;
	}
	q.done++;
}

// Runs what stream `target` needs up to position `pos` (and nothing else), in the policy's order.
inline void run_until(int target, uint64_t pos)
{
	State &S = state();
	if (S.running)
		fatal("a sync point inside a running closure");
	const size_t ns = S.streams.size();
	std::vector<uint64_t> need(ns, 0), scanned(ns, 0);
	need[(size_t)target] = pos;
	if (S.policy == EAGER)
		for (size_t k = 0; k < ns; k++)
			need[k] = std::max(need[k], S.streams[k]->enq);
	for (bool changed = true; changed;)
	{
		changed = false;
		for (size_t k = 0; k < ns; k++)
		{
			Stream &q = *S.streams[k];
			for (uint64_t j = std::max(q.done, scanned[k]); j < need[k]; j++)
			{
				const Op &op = q.q[(size_t)(j - q.done)];
				if (!op.fn && op.wait_pos > need[(size_t)op.wait_stream])
					need[(size_t)op.wait_stream] = op.wait_pos, changed = true;
			}
			scanned[k] = std::max(scanned[k], need[k]);
		}
	}
	std::vector<size_t> ready;
	while (S.streams[(size_t)target]->done < pos)
	{
		ready.clear();
		bool popped = false;
		uint64_t first = ~0ull; // the earliest operation still needed (a policy that takes a later one reorders)
		for (size_t k = 0; k < ns; k++)
		{
			Stream &q = *S.streams[k];
			if (q.done >= need[k])
				continue;
			const Op &h = q.q.front();
			first = std::min(first, h.seq);
			if (h.fn)
				ready.push_back(k);
			else if (S.streams[(size_t)h.wait_stream]->done >= h.wait_pos)
				run_op(q), popped = true; // (a satisfied marker does nothing: drop it at once)
		}
		if (popped)
			continue;
		if (ready.empty())
			fatal("deadlock: a needed stream waits for an operation that can never run");
		size_t pick = ready[0];
		if (S.policy == RANDOM)
		{
			S.rng ^= S.rng << 13, S.rng ^= S.rng >> 7, S.rng ^= S.rng << 17;
			pick = ready[(size_t)(S.rng % ready.size())];
		}
		else
			for (size_t k : ready)
			{
				const uint64_t a = S.streams[k]->q.front().seq, b = S.streams[pick]->q.front().seq;
				if (S.policy == INORDER ? a < b : a > b)
					pick = k;
			}
		if (S.streams[pick]->q.front().seq > first)
			S.out_of_order++;
		run_op(*S.streams[pick]);
	}
}

inline void sync(void *s) { run_until((int)(uintptr_t)s, stream_of(s).enq); }
inline void sync_all()
{
	State &S = state();
	for (size_t k = 0; k < S.streams.size(); k++)
		run_until((int)k, S.streams[k]->enq);
}
inline void stream_destroy(void *s)
{
	sync(s);
}

inline Event *event_create() { return new Event(); }
inline void record(Event *e, void *s)
{
	const uint64_t gen = ++e->gen;
	e->stream = (int)(uintptr_t)s;
	e->timed = false;
	enqueue(s, [e, gen]() {
		if (e->gen == gen) // (the time of the record that is current when this point executes)
			e->t = std::chrono::steady_clock::now(), e->timed = true;
	});
	e->pos = stream_of(s).enq;
}
inline void sync_event(Event *e)
{
	if (e && e->stream >= 0)
		run_until(e->stream, e->pos);
}
inline void destroy_event(Event *e)
{
	sync_event(e); // (its record still refers to it)
	delete e;
}
inline void wait_event(void *s, const Event *e)
{
	State &S = state();
	if (!e || e->stream < 0)
		return;
	if (S.running)
		fatal("a stream wait inside a running closure");
	Stream &q = stream_of(s);
	Op op;
	op.seq = S.seq++, op.wait_stream = e->stream, op.wait_pos = e->pos;
	q.q.push_back(std::move(op));
	q.enq++;
}
inline float elapsed_ms(const Event *a, const Event *b)
{
	if (!a || !b || !a->timed || !b->timed) // (hipEventElapsedTime on a record that has not executed: an error, read as 0)
		return 0.0f;
	return std::chrono::duration<float, std::milli>(b->t - a->t).count();
}

// a copy whose source the host may reuse as soon as the call returns: its bytes are taken now
inline void h2d(void *d, const void *h, size_t n, void *s)
{
	auto bytes = std::make_shared<std::vector<unsigned char>>((const unsigned char *)h, (const unsigned char *)h + n);
	enqueue(s, [d, bytes]() { memcpy(d, bytes->data(), bytes->size()); });
}
inline void copy(void *dst, const void *src, size_t n, void *s)
{
	enqueue(s, [dst, src, n]() { memmove(dst, src, n); });
}

inline void set_schedule(int policy, unsigned seed)
{
	sync_all();
	State &S = state();
	S.policy = policy, S.rng = 0x9E3779B97F4A7C15ull ^ ((uint64_t)seed * 0xBF58476D1CE4E5B9ull);
	if (!S.rng)
		S.rng = 1;
	S.ran = 0, S.out_of_order = 0, S.shadow_packet_launches = 0;
}
} // namespace emu_streams

// the launcher's first statement: outside a running closure, enqueue `call` (the same launcher with the same, copied
// arguments) on stream `s` and return; inside one, fall through to the body
#define EMU_DEFER(s, call)                                                   \
	do                                                                       \
	{                                                                        \
		if (emu_streams::deferring())                                        \
		{                                                                    \
			emu_streams::enqueue((s), [=]() { call; });                      \
			return;                                                          \
		}                                                                    \
	} while (0)
#else
#define EMU_DEFER(s, call) \
	do                     \
	{                      \
	} while (0)
#endif
