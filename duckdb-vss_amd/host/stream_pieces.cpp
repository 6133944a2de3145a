// A vss_read_cb over a serialized index held as consecutive pieces (bench.py's index cache: the stream header, the
// vectors — regenerated from their seeds, in device memory — and the cached graph part), so that vss_load reads a
// 10M-node stream without one host-language call per node.
#include <cstdint>
#include <cstring>

extern "C" {

typedef int (*copy_d2h_fn)(void *dst, const void *src, size_t bytes, int kind); // hipMemcpy

struct StreamPieces {
	const uint8_t *ptr[4];
	uint64_t len[4];
	int32_t on_device[4];
	int32_t count;
	int32_t at;
	uint64_t off;
	copy_d2h_fn copy;
};

int stream_pieces_read(void *ctx, void *data, uint64_t size) {
	StreamPieces *s = static_cast<StreamPieces *>(ctx);
	uint8_t *dst = static_cast<uint8_t *>(data);
	while (size) {
		if (s->at >= s->count)
			return 0;
		const uint64_t left = s->len[s->at] - s->off, n = size < left ? size : left;
		if (s->on_device[s->at]) {
			if (s->copy(dst, s->ptr[s->at] + s->off, n, 2 /* hipMemcpyDeviceToHost */) != 0)
				return 0;
		} else {
			std::memcpy(dst, s->ptr[s->at] + s->off, n);
		}
		dst += n, size -= n, s->off += n;
		if (s->off == s->len[s->at])
			s->at++, s->off = 0;
	}
	return 1;
}
}
