// display_jpeg.h — baseline JPEG of the display stage's RGBA8 image, encoded on the device (settings "display_jpeg_*",
// include/rfwhip.h).  Included by kernels.hip inside namespace rtk, behind display_grade.h: the device kernels
// (k_jpeg_blocks, k_jpeg_entropy, k_jpeg_offsets, k_jpeg_pack; at the end of this file) and the host emulation (kernels_emu.inc) run
// the same items.  Everything is integer arithmetic: the stream is defined byte for byte (rfwhip.h, rfwhip_read_display_jpeg).
//
// BLOCKS  MCU m (raster order) holds bpm = 3 ("444": Y, Cb, Cr of 8 x 8 pixels) or 6 ("420": Y00, Y01, Y10, Y11, Cb, Cr of 16 x 16)
//   blocks; block b = m bpm + k.  The pixel coordinates are clamped to the image (edge replication of RGB, before the conversion).
//   jp_ycc: Y = (19595 R + 38470 G + 7471 B + 32768) >> 16, Cb = (-11059 R - 21709 G + 32768 B + 8421375) >> 16,
//   Cr = (32768 R - 27439 G - 5329 B + 8421375) >> 16; "420": Cb, Cr = (a + b + c + d + 2) >> 2 over 2 x 2.
//   X = block - 128;  T = (K X + 512) >> 10 (jp_col, per column);  S = T K^T (jp_row, per row);
//   q = sgn(S) ((|S| + (Q << 15)) / (Q << 16)) (jp_quant), stored as int16 in zigzag order, 128 bytes per block.
// ENTROPY  jp_encode_block writes a block's Huffman code, most significant bit first, into a strip of JP_STRIP_WORDS 32-bit words (at
//   most 1658 bits: 20 of the DC difference, 63 x 26 of the AC coefficients) and answers its length in bits.  The DC predictor is
//   the previous block of the same component in the same restart interval, 0 at its start (jp_prev_block).
// INTERVALS  interval i = the MCUs [i Ri, min((i + 1) Ri, mcus)); its bytes — padded with 1-bits, a 0x00 behind every 0xFF — go
//   into a slot of the scratch buffer that begins at first_block JP_BLOCK_BYTES + 3 i and holds the worst case.
// Every index that depends on data is bounded: jp_put drops words past the strip, the categories are clamped to the tables.
#pragma once

RT_FN uint32_t jp_ycc(uint32_t rgba)
{
	const int R = (int)(rgba & 255u), G = (int)((rgba >> 8) & 255u), B = (int)((rgba >> 16) & 255u);
	const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
	const int Cb = (-11059 * R - 21709 * G + 32768 * B + 8421375) >> 16;
	const int Cr = (32768 * R - 27439 * G - 5329 * B + 8421375) >> 16;
	return (uint32_t)Y | ((uint32_t)Cb << 8) | ((uint32_t)Cr << 16);
}
RT_FN uint32_t jp_mcu_size(const JpegView &v) { return v.sub ? 16u : 8u; }
// the packed Y / Cb / Cr of pixel (x, y) of MCU m, the coordinates clamped to the image
RT_FN uint32_t jp_pixel(const JpegView &v, uint32_t m, uint32_t x, uint32_t y)
{
	const uint32_t M = jp_mcu_size(v), my = m / v.mcus_x, mx = m - my * v.mcus_x;
	const uint32_t gx = mx * M + x < v.W ? mx * M + x : v.W - 1u, gy = my * M + y < v.H ? my * M + y : v.H - 1u;
	return jp_ycc(v.rgba[(size_t)gy * v.W + gx]);
}
// sample (x, y) of block k of an MCU whose M x M packed pixels are t[y M + x]
template <class T> RT_FN int jp_sample(const T *t, uint32_t sub, uint32_t k, uint32_t x, uint32_t y)
{
	if (!sub)
		return (int)((t[y * 8u + x] >> (8u * k)) & 255u);
	if (k < 4u)
		return (int)(t[((k >> 1) * 8u + y) * 16u + (k & 1u) * 8u + x] & 255u);
	const uint32_t sh = 8u * (k - 3u), o = (2u * y) * 16u + 2u * x;
	return (int)((((t[o] >> sh) & 255u) + ((t[o + 1u] >> sh) & 255u) + ((t[o + 16u] >> sh) & 255u) + ((t[o + 17u] >> sh) & 255u) + 2u) >> 2);
}
// T[u] = (sum_y K[u][y] X[y] + 512) >> 10 for one column X of samples (128 not yet subtracted)
RT_FN void jp_col(const JpegTables &tab, const int X[8], int T[8])
{
	for (int u = 0; u < 8; u++)
	{
		int a = 512;
		for (int y = 0; y < 8; y++)
			a += tab.K[u * 8 + y] * (X[y] - 128);
		T[u] = a >> 10;
	}
}
// S[v] = sum_x T[x] K[v][x] for one row T
RT_FN void jp_row(const JpegTables &tab, const int T[8], int S[8])
{
	for (int v = 0; v < 8; v++)
	{
		int a = 0;
		for (int x = 0; x < 8; x++)
			a += T[x] * tab.K[v * 8 + x];
		S[v] = a;
	}
}
RT_FN int jp_quant(int S, uint32_t Q)
{
	const uint32_t a = (uint32_t)(S < 0 ? -S : S), q = (a + (Q << 15)) / (Q << 16);
	return S < 0 ? -(int)q : (int)q;
}
// one whole block from its MCU's packed pixels (the emulation; the device runs the same steps on eight lanes): zz[0 .. 63]
template <class T> RT_FN void jp_block_item(const JpegView &v, const T *t, uint32_t k, int16_t *zz)
{
	const JpegTables &tab = *v.tab;
	const uint32_t table = v.sub ? (k >= 4u) : (k >= 1u);
	int Tm[64];
	for (uint32_t x = 0; x < 8u; x++)
	{
		int X[8], Tc[8];
		for (uint32_t y = 0; y < 8u; y++)
			X[y] = jp_sample(t, v.sub, k, x, y);
		jp_col(tab, X, Tc);
		for (int u = 0; u < 8; u++)
			Tm[u * 8 + (int)x] = Tc[u];
	}
	for (int u = 0; u < 8; u++)
	{
		int S[8];
		jp_row(tab, Tm + u * 8, S);
		for (int c = 0; c < 8; c++)
			zz[tab.izz[u * 8 + c] & 63u] = (int16_t)jp_quant(S[c], v.q[table][u * 8 + c]);
	}
}

// ---- entropy coding ----
struct JpBits
{
	uint32_t *w;	 // the strip: word i at w[i stride]
	uint32_t stride; // (the device interleaves the lanes' strips)
	uint32_t n;		 // words written
	uint64_t acc;	 // `have` pending bits in its low end
	uint32_t have, bits;
};
RT_FN void jp_put(JpBits &b, uint32_t code, uint32_t len) // len <= 26
{
	b.acc = (b.acc << len) | (uint64_t)code, b.have += len, b.bits += len;
	if (b.have >= 32u)
	{
		b.have -= 32u;
		if (b.n < JP_STRIP_WORDS)
			b.w[(size_t)b.n * b.stride] = (uint32_t)(b.acc >> b.have);
		b.n++;
		b.acc &= (1ull << b.have) - 1ull;
	}
}
RT_FN uint32_t jp_category(int v) // bits of |v|
{
	uint32_t a = (uint32_t)(v < 0 ? -v : v), s = 0u;
	for (; a; a >>= 1)
		s++;
	return s;
}
// the block whose DC coefficient predicts block b's, or ~0u at the start of its restart interval (first = the interval's first block)
RT_FN uint32_t jp_prev_block(uint32_t sub, uint32_t b, uint32_t first)
{
	const uint32_t k = b % (sub ? 6u : 3u);
	const uint32_t back = !sub ? 3u : k == 0u ? 3u : k < 4u ? 1u : 6u;
	return b >= first + back ? b - back : ~0u;
}
// the code of one block: its coefficients zz[0 .. 63] in zigzag order, the predictor, table 0 (luminance) | 1 -> the bits written
RT_FN uint32_t jp_encode_block(const JpegTables &tab, const int16_t *zz, int pred, uint32_t table, uint32_t *strip, uint32_t stride)
{
	JpBits b;
	b.w = strip, b.stride = stride, b.n = 0u, b.acc = 0ull, b.have = 0u, b.bits = 0u;
	const int d = (int)zz[0] - pred;
	uint32_t s = jp_category(d);
	s = s < 11u ? s : 11u;
	uint32_t h = tab.dc[table][s];
	jp_put(b, ((h & 0xFFFFu) << s) | ((uint32_t)(d < 0 ? d - 1 : d) & ((1u << s) - 1u)), (h >> 16) + s);
	uint32_t run = 0u;
	for (int k = 1; k < 64; k++)
	{
		const int a = (int)zz[k];
		if (a == 0)
		{
			run++;
			continue;
		}
		for (; run > 15u; run -= 16u)
			h = tab.ac[table][0xF0], jp_put(b, h & 0xFFFFu, h >> 16);
		s = jp_category(a);
		s = s < 10u ? s : 10u;
		h = tab.ac[table][run * 16u + s];
		jp_put(b, ((h & 0xFFFFu) << s) | ((uint32_t)(a < 0 ? a - 1 : a) & ((1u << s) - 1u)), (h >> 16) + s);
		run = 0u;
	}
	if (run)
		h = tab.ac[table][0], jp_put(b, h & 0xFFFFu, h >> 16);
	if (b.have && b.n < JP_STRIP_WORDS)
		b.w[(size_t)b.n * b.stride] = (uint32_t)(b.acc << (32u - b.have));
	const uint32_t cap = JP_STRIP_WORDS * 32u;
	return b.bits < cap ? b.bits : cap;
}
RT_FN uint32_t jp_interval_first(const JpegView &v, uint32_t i) { return i * v.ri * v.bpm; } // (i ri <= mcus)
RT_FN uint32_t jp_interval_blocks(const JpegView &v, uint32_t i)
{
	const uint32_t m0 = i * v.ri;
	return (v.mcus - m0 < v.ri ? v.mcus - m0 : v.ri) * v.bpm;
}
RT_FN size_t jp_slot(const JpegView &v, uint32_t i) { return (size_t)jp_interval_first(v, i) * JP_BLOCK_BYTES + 3u * (size_t)i; }
// the two bytes behind interval i: RSTn, or EOI behind the last one
RT_FN uint32_t jp_marker(const JpegView &v, uint32_t i) { return i + 1u < v.intervals ? 0xD0u + (i & 7u) : 0xD9u; }
// the record behind the scan over the intervals' byte counts: `total` = the whole stream, header and markers included
RT_FN void jp_record(const JpegView &v, uint64_t total, uint32_t stuffed)
{
	JpegRecord r;
	r.bytes = total > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)total, r.intervals = v.intervals, r.mcus = v.mcus, r.blocks = v.blocks;
	r.stuffed = stuffed, r.overflow = total > (uint64_t)v.cap ? 1u : 0u, r.header = JP_HEADER, r.pad = 0u;
	*v.rec = r;
}

#if defined(RT_DEVICE_BUILD)
// ---- k_jpeg_blocks: a workgroup of JP_THREADS = 192 owns JP_GROUP = 24 blocks: 8 MCUs of "444" or 4 of "420", 64 x 8 or 64 x 16
// pixels.  It stages their packed Y / Cb / Cr in LDS — a thread and round one pixel, consecutive threads along a row across the
// group's MCUs: 256 contiguous bytes of RGBA8 while the MCUs share a row — then eight lanes share a block: lane j transforms column j,
// the eight exchange T through LDS, lane j transforms and quantises row j into the zigzag order in LDS, and stores coefficients
// 8 j .. 8 j + 7 as one 16-byte row: a block leaves as 128 contiguous bytes.  Groups past the last MCU idle (no clamping onto a
// neighbour); every thread reaches every barrier. ----
constexpr uint32_t JP_THREADS = 192u, JP_GROUP = 24u;
__global__ void __launch_bounds__(JP_THREADS) k_jpeg_blocks(const JpegView v)
{
	__shared__ uint32_t s_px[1024];
	__shared__ int s_t[JP_GROUP][64];
	__shared__ __attribute__((aligned(16))) int16_t s_q[JP_GROUP][64];
	const uint32_t M = jp_mcu_size(v), per = JP_GROUP / v.bpm, m0 = blockIdx.x * per, row = per * M;
	for (uint32_t i = threadIdx.x; i < row * M; i += JP_THREADS)
	{
		const uint32_t y = i / row, r = i - y * row, m = r / M, x = r - m * M;
		if (m0 + m < v.mcus)
			s_px[(m * M + y) * M + x] = jp_pixel(v, m0 + m, x, y);
	}
	__syncthreads();
	const uint32_t g = threadIdx.x >> 3, j = threadIdx.x & 7u, m = g / v.bpm, k = g - m * v.bpm;
	const bool live = m0 + m < v.mcus;
	const JpegTables &tab = *v.tab;
	if (live)
	{
		int X[8], T[8];
		for (uint32_t y = 0; y < 8u; y++)
			X[y] = jp_sample(s_px + m * M * M, v.sub, k, j, y);
		jp_col(tab, X, T);
		for (int u = 0; u < 8; u++)
			s_t[g][u * 8 + (int)j] = T[u];
	}
	__syncthreads();
	if (live)
	{
		const uint32_t table = v.sub ? (k >= 4u) : (k >= 1u);
		int S[8];
		jp_row(tab, &s_t[g][j * 8u], S);
		for (uint32_t c = 0; c < 8u; c++)
			s_q[g][tab.izz[j * 8u + c] & 63u] = (int16_t)jp_quant(S[c], v.q[table][j * 8u + c]);
	}
	__syncthreads();
	if (live)
		*(uint4 *)(v.coef + ((size_t)(m0 + m) * v.bpm + k) * 64u + 8u * j) = *(const uint4 *)&s_q[g][8u * j];
}

// ---- k_jpeg_entropy: one wave64 per restart interval, one lane per block, the interval walked in chunks of 64 blocks.  A lane
// writes its block's code into a strip of its own (LDS, the lanes' strips interleaved word by word); a wave prefix sum of the
// lengths places the blocks behind the `cb` bits the previous chunk left over; every lane then ORs its strip, shifted, into the
// chunk's bit string (integer LDS atomics: OR commutes, and only a block's first and last word meet a neighbour's).  The string's
// whole bytes leave 64 per round: a ballot counts the 0xFF bytes in front of a lane, and the lane stores its byte, and a 0x00 behind
// an 0xFF, at its place in the interval's slot.  The last chunk pads with 1-bits.  Lanes past the interval's last block idle. ----
constexpr uint32_t JP_MERGE_WORDS = 64u * JP_STRIP_WORDS + 2u;
__global__ void __launch_bounds__(64) k_jpeg_entropy(const JpegView v)
{
	__shared__ uint32_t s_strip[JP_STRIP_WORDS * 64u];
	__shared__ uint32_t s_merge[JP_MERGE_WORDS];
	const uint32_t i = blockIdx.x, lane = threadIdx.x;
	const uint32_t first = jp_interval_first(v, i), n = jp_interval_blocks(v, i);
	const JpegTables &tab = *v.tab;
	uint8_t *slot = v.slots + jp_slot(v, i);
	uint32_t out = 0u, stuffed = 0u, cb = 0u, cv = 0u; // wave-uniform
	for (uint32_t c0 = 0; c0 < n; c0 += 64u)
	{
		const bool live = c0 + lane < n;
		const bool last = c0 + 64u >= n;
		uint32_t len = 0u;
		if (live)
		{
			const uint32_t b = first + c0 + lane, k = b % v.bpm, p = jp_prev_block(v.sub, b, first);
			const int pred = p == ~0u ? 0 : (int)v.coef[(size_t)p * 64u];
			len = jp_encode_block(tab, v.coef + (size_t)b * 64u, pred, v.sub ? (k >= 4u) : (k >= 1u), s_strip + lane, 64u);
		}
		uint32_t end = len; // inclusive prefix sum over the wave
		for (uint32_t d = 1u; d < 64u; d <<= 1)
		{
			const uint32_t o = (uint32_t)__shfl_up((int)end, d, 64);
			if (lane >= d)
				end += o;
		}
		const uint32_t total = cb + (uint32_t)__shfl((int)end, 63, 64); // <= 7 + 64 x 1664 bits: inside s_merge
		const uint32_t at = cb + end - len;
		const uint32_t padded = last ? (total + 7u) & ~7u : total;
		for (uint32_t w = lane; w < (padded + 31u) / 32u + 1u && w < JP_MERGE_WORDS; w += 64u)
			s_merge[w] = 0u;
		__syncthreads();
		if (lane == 0u && cb)
			atomicOr(&s_merge[0], cv << (32u - cb));
		if (lane == 0u && padded > total) // 1-bits up to the byte: total & 31 != 0 here
			atomicOr(&s_merge[total >> 5], ((1u << (padded - total)) - 1u) << (32u - (total & 31u) - (padded - total)));
		for (uint32_t w = 0; w * 32u < len; w++)
		{
			const uint32_t x = s_strip[w * 64u + lane], p = at + w * 32u, sh = p & 31u;
			atomicOr(&s_merge[p >> 5], x >> sh);
			if (sh)
				atomicOr(&s_merge[(p >> 5) + 1u], x << (32u - sh));
		}
		__syncthreads();
		const uint32_t bytes = padded >> 3;
		for (uint32_t j0 = 0; j0 < bytes; j0 += 64u)
		{
			const uint32_t j = j0 + lane;
			const bool have = j < bytes;
			const uint32_t byte = have ? (s_merge[j >> 2] >> (24u - 8u * (j & 3u))) & 255u : 0u;
			const unsigned long long ff = __ballot(have && byte == 255u);
			const uint32_t before = (uint32_t)__popcll(ff & ((1ull << lane) - 1ull));
			if (have)
			{
				slot[out + lane + before] = (uint8_t)byte;
				if (byte == 255u)
					slot[out + lane + before + 1u] = 0u;
			}
			const uint32_t round = bytes - j0 < 64u ? bytes - j0 : 64u, nff = (uint32_t)__popcll(ff);
			out += round + nff, stuffed += nff;
		}
		cb = padded & 7u; // (0 behind the last chunk)
		cv = cb ? (s_merge[bytes >> 2] >> (24u - 8u * (bytes & 3u)) & 255u) >> (8u - cb) : 0u;
		__syncthreads();
	}
	if (lane == 0u)
		v.counts[2u * i] = out, v.counts[2u * i + 1u] = stuffed;
}

// ---- k_jpeg_offsets: one workgroup.  Thread t adds the bytes (+ 2: the marker) of a contiguous run of intervals, thread 0 scans
// the BLOCK sums, every thread writes its run's exclusive offsets, thread 0 the record. ----
__global__ void __launch_bounds__(BLOCK) k_jpeg_offsets(const JpegView v)
{
	__shared__ unsigned long long s_sum[BLOCK];
	__shared__ uint32_t s_stuffed[BLOCK];
	const uint32_t t = threadIdx.x, per = (v.intervals + BLOCK - 1u) / BLOCK;
	const uint32_t a = t * per < v.intervals ? t * per : v.intervals, b = a + per < v.intervals ? a + per : v.intervals;
	unsigned long long sum = 0ull;
	uint32_t st = 0u;
	for (uint32_t i = a; i < b; i++)
		sum += (unsigned long long)v.counts[2u * i] + 2ull, st += v.counts[2u * i + 1u];
	s_sum[t] = sum, s_stuffed[t] = st;
	__syncthreads();
	if (t == 0u)
	{
		unsigned long long run = JP_HEADER;
		uint32_t all = 0u;
		for (uint32_t k = 0; k < (uint32_t)BLOCK; k++)
		{
			const unsigned long long x = s_sum[k];
			s_sum[k] = run, run += x, all += s_stuffed[k];
		}
		jp_record(v, run, all);
	}
	__syncthreads();
	unsigned long long off = s_sum[t];
	for (uint32_t i = a; i < b; i++)
		v.offsets[i] = off > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)off, off += (unsigned long long)v.counts[2u * i] + 2ull;
}

// ---- k_jpeg_pack: a wave per interval copies the slot's bytes to their place behind the header and appends the marker; with the
// record's overflow flag set it writes nothing (every offset + length is then unchecked against cap, so none is used). ----
__global__ void __launch_bounds__(BLOCK) k_jpeg_pack(const JpegView v)
{
	const uint32_t i = blockIdx.x * (BLOCK / 64u) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (i >= v.intervals || v.rec->overflow)
		return;
	const uint8_t *slot = v.slots + jp_slot(v, i);
	const uint32_t n = v.counts[2u * i];
	uint8_t *dst = v.out + v.offsets[i];
	for (uint32_t j = lane; j < n; j += 64u)
		dst[j] = slot[j];
	if (lane == 0u)
		dst[n] = 0xFFu, dst[n + 1u] = (uint8_t)jp_marker(v, i);
}

void launch_jpeg_blocks(const JpegView &v, stream_t s)
{
	const uint32_t per = JP_GROUP / v.bpm;
	hipLaunchKernelGGL(k_jpeg_blocks, dim3((v.mcus + per - 1u) / per), dim3(JP_THREADS), 0, (hipStream_t)s, v);
}
void launch_jpeg_entropy(const JpegView &v, stream_t s) { hipLaunchKernelGGL(k_jpeg_entropy, dim3(v.intervals), dim3(64), 0, (hipStream_t)s, v); }
void launch_jpeg_offsets(const JpegView &v, stream_t s) { hipLaunchKernelGGL(k_jpeg_offsets, dim3(1), dim3(BLOCK), 0, (hipStream_t)s, v); }
void launch_jpeg_pack(const JpegView &v, stream_t s)
{
	hipLaunchKernelGGL(k_jpeg_pack, dim3((v.intervals + BLOCK / 64u - 1u) / (BLOCK / 64u)), dim3(BLOCK), 0, (hipStream_t)s, v);
}
#endif
