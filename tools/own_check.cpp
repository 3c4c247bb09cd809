// own_check.cpp - csrc/device_own.h as a program of its own on the CPU, under AddressSanitizer + UBSan
// (tests/test_own_cpu.py).  The handful of runtime functions the header calls are defined here on malloc / free, with a
// table of the live blocks - every step compares the header's live counters with it - and a switch that makes the next
// allocation fail.  A double free, a free of something never allocated, a leak at exit: the table or the sanitizer says so.
// With RTLFM_POISON=1 in the environment the poison path is checked as well.
#include "../rtlsdr_amd/csrc/device_own.h"

#include <cstring>
#include <map>
#include <utility>

enum { kDev, kPinned, kEvent };
static std::map<void *, std::pair<int, size_t>> g_live;  // block -> (kind, bytes)
static bool g_fail_next = false;
static int g_frees = 0, g_syncs = 0;

#define CHECK(cond)                                                                    \
	do {                                                                               \
		if (!(cond)) {                                                                 \
			fprintf(stderr, "own_check: %s failed (line %d)\n", #cond, __LINE__);      \
			exit(1);                                                                   \
		}                                                                              \
	} while (0)

static hipError_t stub_alloc(void **p, size_t n, int kind)
{
	if (g_fail_next) { g_fail_next = false; *p = nullptr; return hipErrorOutOfMemory; }
	if (!n) { *p = nullptr; return hipSuccess; }  // (as the runtime: no bytes, no block)
	*p = malloc(n);
	if (!*p) return hipErrorOutOfMemory;
	memset(*p, 0x11, n);
	g_live[*p] = {kind, n};
	return hipSuccess;
}
static hipError_t stub_free(void *p, int kind)
{
	auto it = g_live.find(p);
	CHECK(it != g_live.end());  // (freed twice, or never allocated - or an interior pointer)
	CHECK(it->second.first == kind);
	g_live.erase(it);
	free(p);
	g_frees++;
	return hipSuccess;
}
extern "C" {
hipError_t (hipMalloc)(void **p, size_t n) { return stub_alloc(p, n, kDev); }  // (in parentheses: the header's macro)
hipError_t hipFree(void *p) { return stub_free(p, kDev); }
hipError_t hipHostMalloc(void **p, size_t n, unsigned int) { return stub_alloc(p, n, kPinned); }
hipError_t hipHostFree(void *p) { return stub_free(p, kPinned); }
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) { return stub_alloc((void **)e, 8, kEvent); }
hipError_t hipEventDestroy(hipEvent_t e) { return stub_free((void *)e, kEvent); }
hipError_t hipMemset(void *p, int v, size_t n) { memset(p, v, n); return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t q) { g_syncs += q != nullptr; return hipSuccess; }  // (the null stream: the poison fill's)
const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
}

// the header's counters against the table
static void same_counts()
{
	long n[3] = {0, 0, 0};
	for (auto &kv : g_live) n[kv.second.first]++;
	for (int k = 0; k < 3; k++) CHECK(rtl_own::live(k).load() == n[k]);
}
static long live_dev() { return rtl_own::live(kDev).load(); }

struct Handle {  // what the library's handles look like: several owners and plain state
	DevBuf<int> a;
	DevBuf<float> b[2];
	PinnedBuf<short> pin;
	Event ev;
	int x = 0;
};

int main()
{
	const bool poison = rtl_debug::poison_on();
	hipStream_t q = (hipStream_t)&g_syncs;  // (never looked into)
	same_counts();
	{  // alloc, destroy
		DevBuf<int> d;
		CHECK(!d && d.capacity() == 0);
		CHECK(d.alloc(10) == 0 && d && d.capacity() == 10 && live_dev() == 1);
		same_counts();
		const unsigned char want = poison ? 0xA5 : 0x11;  // (RTLFM_POISON=1: every byte filled before use)
		for (size_t i = 0; i < 10 * sizeof(int); i++) CHECK(((unsigned char *)d.get())[i] == want);
		int *p = d;
		CHECK(d.alloc(99) == 0 && d.get() == p && d.capacity() == 10);  // (holds something: nothing to do)
		DevBuf<int> z;
		PinnedBuf<short> hz;
		CHECK(z.alloc(0) == 0 && !z && z.capacity() == 0 && hz.alloc(0) == 0 && !hz && z.adopt(nullptr, 7) == 0 && z.capacity() == 0);
		same_counts();  // (nothing held: nothing counted)
		PinnedBuf<short> h;
		Event e;
		CHECK(h.alloc(5) == 0 && e.create(hipEventDisableTiming) == 0 && (hipEvent_t)e);
		same_counts();
		CHECK(rtl_own::live(kPinned) == 1 && rtl_own::live(kEvent) == 1);
	}
	same_counts();
	CHECK(g_live.empty());
	{  // move construction and assignment: the source is left empty, nothing is freed twice
		DevBuf<int> a;
		CHECK(a.alloc(4) == 0);
		int *p = a;
		DevBuf<int> b(std::move(a));
		CHECK(!a && a.capacity() == 0 && b.get() == p && b.capacity() == 4 && !b.is_alias());
		DevBuf<int> c;
		CHECK(c.alloc(2) == 0);
		const int frees = g_frees;
		c = std::move(b);  // (c's own block goes)
		CHECK(g_frees == frees + 1 && !b && c.get() == p && live_dev() == 1);
		same_counts();
		Event e, f;
		CHECK(e.create() == 0);
		f = std::move(e);
		CHECK(!(hipEvent_t)e && (hipEvent_t)f);
		same_counts();
	}
	same_counts();
	CHECK(g_live.empty());
	{  // grow
		DevBuf<int> d;
		CHECK(d.grow(8, q) == 0 && d.capacity() == 8);
		int *p = d;
		const int syncs = g_syncs, frees = g_frees;
		CHECK(d.grow(8, q) == 0 && d.grow(3, q) == 0 && d.get() == p && g_syncs == syncs && g_frees == frees);  // (enough: untouched)
		CHECK(d.grow(16, q) == 0 && d.capacity() == 16 && g_syncs == syncs + 1 && g_frees == frees + 1);     // (waited, the old block freed once)
		same_counts();
		g_fail_next = true;
		CHECK(d.grow(64, q) == -ENOMEM && !d && d.capacity() == 0 && g_frees == frees + 2 && live_dev() == 0);  // (empty, never short)
		same_counts();
		CHECK(d.grow(64, q) == 0 && d.capacity() == 64 && g_frees == frees + 2);
		g_fail_next = true;
		PinnedBuf<short> h;
		CHECK(h.alloc(4) == -ENOMEM && !h && h.alloc(4) == 0 && h.capacity() == 4);
		same_counts();
	}
	same_counts();
	CHECK(g_live.empty());
	{  // a copy of a struct of owners is all aliases
		Handle h;
		CHECK(h.a.alloc(10) == 0 && h.b[0].alloc(3) == 0 && h.pin.alloc(6) == 0 && h.ev.create() == 0);
		same_counts();
		const int frees = g_frees;
		{
			Handle v = h;
			v.x = 1;
			CHECK(v.a.get() == h.a.get() && v.a.capacity() == 10 && v.a.is_alias() && v.pin.get() == h.pin.get());
			CHECK((hipEvent_t)v.ev == (hipEvent_t)h.ev);
			CHECK(v.a.grow(11, q) == -EINVAL && v.a.get() == h.a.get());  // (a view must not allocate)
			CHECK(v.b[1].alloc(4) == -EINVAL && !v.b[1]);                 // ... nor fill what the handle has not got
			CHECK(v.b[1].adopt(nullptr, 0) == -EINVAL);
			PinnedBuf<short> none_pinned, p2 = none_pinned;
			CHECK(p2.alloc(100) == -EINVAL && !p2);
			Event none = Event();
			Event e2 = none;
			CHECK(e2.create() == -EINVAL);
			CHECK(v.a.alloc(10) == 0 && v.a.grow(10, q) == 0);  // (there already: nothing to do is not an allocation)
			same_counts();
			// the one thing a view may do: forget the handle's block and own one of its own
			v.b[0].reset();
			CHECK(!v.b[0] && !v.b[0].is_alias() && h.b[0] && g_frees == frees);
			CHECK(v.b[0].alloc(5) == 0 && v.b[0].get() != h.b[0].get() && live_dev() == 3);
			same_counts();
		}
		CHECK(g_frees == frees + 1 && live_dev() == 2);  // (the view's own block and nothing of the handle's)
		same_counts();
		h.a.get()[9] = 7;  // (still there: the sanitizer would say)
		DevBuf<int> off = h.a.alias(4);
		CHECK(off.get() == h.a.get() + 4 && off.capacity() == 6 && off.is_alias());
		CHECK(!DevBuf<int>().alias(3));
	}
	same_counts();
	CHECK(g_live.empty());
	{  // adopt: a block somebody else allocated, freed once; an alias into it, replaced by an owner
		void *blk = nullptr;
		CHECK(hipMalloc(&blk, 64) == hipSuccess);  // (the placement search's)
		DevBuf<short> own[2];
		CHECK(own[0].adopt(blk, 32) == 0 && own[0].capacity() == 32 && live_dev() == 1);
		own[1] = own[0].alias(16);
		same_counts();
		void *blk2 = nullptr;
		CHECK(hipMalloc(&blk2, 32) == hipSuccess);
		own[1].reset();
		CHECK(own[1].adopt(blk2, 16) == 0 && live_dev() == 2);
		same_counts();
	}
	same_counts();
	CHECK(g_live.empty());
	for (int k = 0; k < 3; k++) CHECK(rtl_own::live(k).load() == 0);
	printf("own_check: ok (%d frees%s)\n", g_frees, poison ? ", poisoned" : "");
	return 0;
}
