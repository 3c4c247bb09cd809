// device_own.h - who owns what on the device: DevBuf<T> (hipMalloc), PinnedBuf<T> (hipHostMalloc) and Event.
// Host code only (<hip/hip_runtime_api.h>; plain g++ compiles it: tools/own_check.cpp).
//
// Each converts to its raw form, so launch sites and pointer arithmetic read as with raw pointers, and frees what it
// holds when it goes.  COPYING one - and so copying a struct of them, as the stream-range views do - yields an ALIAS: the
// same memory, owned by nobody.  An alias frees nothing, and alloc / grow / adopt / create through one fail with -EINVAL:
// "views must not allocate" is a checked condition.  reset() on an alias forgets the memory and leaves an empty owner.
// Moving takes everything over and leaves the source empty; copy assignment does not exist.
//
// Errors are the library's: -ENOMEM for hipErrorOutOfMemory, -EIO otherwise, with a line on stderr under the unit's name
// (OWN_UNIT, defined by a unit in front of this header where it is not "rtlfm_hip").
//
// RTLFM_POISON=1 (debug_poison.h has the LDS half and the why): every device allocation is filled with 0xA5 before use -
// DevBuf's, and through the macro at the end every plain hipMalloc of a unit that includes this.
#pragma once
#include <hip/hip_runtime_api.h>
#include <atomic>
#include <cerrno>
#include <cstddef>
#include <cstdio>
#include <cstdlib>

namespace rtl_debug {

inline bool poison_on()
{
	static const bool on = [] { const char *e = getenv("RTLFM_POISON"); return e && *e && *e != '0'; }();
	return on;
}

inline hipError_t poison_malloc(void **p, size_t n)
{
	const hipError_t e = (hipMalloc)(p, n);  // (the parentheses keep the macro below out of this call)
	if (e == hipSuccess && n && poison_on()) {
		if ((hipMemset)(*p, 0xA5, n) != hipSuccess || hipStreamSynchronize(nullptr) != hipSuccess) return hipErrorUnknown;
	}
	return e;
}

}  // namespace rtl_debug

#ifndef OWN_UNIT
#define OWN_UNIT "rtlfm_hip"
#endif

namespace rtl_own {

// what the three types hold right now, process-wide: 0 device allocations, 1 pinned allocations, 2 events (rtlfm_debug_live)
inline std::atomic<long> &live(int kind)
{
	static std::atomic<long> n[3];
	return n[kind];
}

// (static, not inline: each unit's copy speaks under that unit's name)
static int failed(const char *what, hipError_t e, bool quiet = false)
{
	if (!quiet) fprintf(stderr, OWN_UNIT ": %s -> %s (%s)\n", what, hipGetErrorString(e), __FILE__);
	return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
}
static int through_alias(const char *what)
{
	fprintf(stderr, OWN_UNIT ": %s through an alias: a view must not allocate (%s)\n", what, __FILE__);
	return -EINVAL;
}

}  // namespace rtl_own

#define OWN_TRY(expr)             \
	do {                          \
		const int r_ = (expr);    \
		if (r_ < 0) return r_;    \
	} while (0)

template <class T> class DevBuf {
	T *p_ = nullptr;
	size_t n_ = 0;  // capacity, elements
	bool alias_ = false;

public:
	DevBuf() = default;
	DevBuf(const DevBuf &o) : p_(o.p_), n_(o.n_), alias_(true) {}
	DevBuf(DevBuf &&o) noexcept : p_(o.p_), n_(o.n_), alias_(o.alias_) { o.p_ = nullptr; o.n_ = 0; }
	DevBuf &operator=(const DevBuf &) = delete;
	DevBuf &operator=(DevBuf &&o) noexcept
	{
		if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; alias_ = o.alias_; o.p_ = nullptr; o.n_ = 0; }
		return *this;
	}
	~DevBuf() { reset(); }

	operator T *() const { return p_; }
	T *get() const { return p_; }
	size_t capacity() const { return n_; }
	bool is_alias() const { return alias_; }

	// the same memory from element off on, owned by nobody
	DevBuf alias(size_t off = 0) const
	{
		DevBuf a;
		a.p_ = p_ ? p_ + off : nullptr; a.n_ = n_ > off ? n_ - off : 0; a.alias_ = true;
		return a;
	}
	// frees (an alias: forgets) and leaves an empty owner
	void reset()
	{
		if (p_ && !alias_) { (void)hipFree(p_); rtl_own::live(0)--; }
		p_ = nullptr; n_ = 0; alias_ = false;
	}
	// n elements unless something is held already (quiet: a failure the caller tolerates leaves no line on stderr)
	int alloc(size_t n, bool quiet = false)
	{
		if (p_) return 0;
		if (alias_) return rtl_own::through_alias("DevBuf::alloc");
		void *q = nullptr;
		const hipError_t e = ::rtl_debug::poison_malloc(&q, n * sizeof(T));
		if (e != hipSuccess) return rtl_own::failed("hipMalloc", e, quiet);
		p_ = static_cast<T *>(q); n_ = p_ ? n : 0;  // (0 bytes: no block, nothing held, nothing counted)
		if (p_) rtl_own::live(0)++;
		return 0;
	}
	// at least n elements.  Short: waits for stream - whatever may still use the old block -, frees it, and reads as
	// empty from then until the new allocation has succeeded (a failure half way leaves no capacity beside freed memory).
	int grow(size_t n, hipStream_t stream)
	{
		if (n <= n_) return 0;
		if (alias_) return rtl_own::through_alias("DevBuf::grow");
		if (p_) {
			const hipError_t e = hipStreamSynchronize(stream);
			if (e != hipSuccess) return rtl_own::failed("hipStreamSynchronize", e);
			reset();
		}
		return alloc(n);
	}
	// takes over a block somebody else allocated (the placement search, rtlfm_place.hip)
	int adopt(void *ptr, size_t elems)
	{
		if (alias_) return rtl_own::through_alias("DevBuf::adopt");
		reset();
		p_ = static_cast<T *>(ptr); n_ = p_ ? elems : 0;
		if (p_) rtl_own::live(0)++;
		return 0;
	}
};

template <class T> class PinnedBuf {
	T *p_ = nullptr;
	size_t n_ = 0;
	bool alias_ = false;

public:
	PinnedBuf() = default;
	PinnedBuf(const PinnedBuf &o) : p_(o.p_), n_(o.n_), alias_(true) {}
	PinnedBuf(PinnedBuf &&o) noexcept : p_(o.p_), n_(o.n_), alias_(o.alias_) { o.p_ = nullptr; o.n_ = 0; }
	PinnedBuf &operator=(const PinnedBuf &) = delete;
	PinnedBuf &operator=(PinnedBuf &&o) noexcept
	{
		if (this != &o) { reset(); p_ = o.p_; n_ = o.n_; alias_ = o.alias_; o.p_ = nullptr; o.n_ = 0; }
		return *this;
	}
	~PinnedBuf() { reset(); }

	operator T *() const { return p_; }
	T *get() const { return p_; }
	size_t capacity() const { return n_; }

	void reset()
	{
		if (p_ && !alias_) { (void)hipHostFree(p_); rtl_own::live(1)--; }
		p_ = nullptr; n_ = 0; alias_ = false;
	}
	int alloc(size_t n)
	{
		if (p_) return 0;
		if (alias_) return rtl_own::through_alias("PinnedBuf::alloc");
		void *q = nullptr;
		const hipError_t e = hipHostMalloc(&q, n * sizeof(T), hipHostMallocDefault);
		if (e != hipSuccess) return rtl_own::failed("hipHostMalloc", e);
		p_ = static_cast<T *>(q); n_ = p_ ? n : 0;
		if (p_) rtl_own::live(1)++;
		return 0;
	}
};

class Event {
	hipEvent_t e_ = nullptr;
	bool alias_ = false;

public:
	Event() = default;
	Event(const Event &o) : e_(o.e_), alias_(true) {}
	Event(Event &&o) noexcept : e_(o.e_), alias_(o.alias_) { o.e_ = nullptr; }
	Event &operator=(const Event &) = delete;
	Event &operator=(Event &&o) noexcept
	{
		if (this != &o) { reset(); e_ = o.e_; alias_ = o.alias_; o.e_ = nullptr; }
		return *this;
	}
	~Event() { reset(); }

	operator hipEvent_t() const { return e_; }

	void reset()
	{
		if (e_ && !alias_) { (void)hipEventDestroy(e_); rtl_own::live(2)--; }
		e_ = nullptr; alias_ = false;
	}
	// created with these flags unless there is one already
	int create(unsigned flags = hipEventDefault)
	{
		if (e_) return 0;
		if (alias_) return rtl_own::through_alias("Event::create");
		const hipError_t e = hipEventCreateWithFlags(&e_, flags);
		if (e != hipSuccess) { e_ = nullptr; return rtl_own::failed("hipEventCreateWithFlags", e); }
		rtl_own::live(2)++;
		return 0;
	}
};

#define hipMalloc(p, n) ::rtl_debug::poison_malloc((void **)(p), (n))
