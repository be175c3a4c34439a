// CPU-only tracing stand-in for the HIP runtime calls the library makes: logs every enqueue (kernel name, grid, block, LDS, stream), copies / memsets
// on host memory, event record / wait.  Nothing runs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
struct dim3 { uint32_t x, y, z; };
static std::map<const void*, std::string> names;
static std::map<const void*, int> ids;
static FILE* out() { static FILE* f = fopen(getenv("TRACE_OUT") ? getenv("TRACE_OUT") : "/dev/stderr", "w"); return f; }
static int id_of(const void* p) { if (!p) return 0; auto it = ids.find(p); if (it != ids.end()) return it->second; int n = (int)ids.size() + 1; ids[p] = n; return n; }
struct Cfg { dim3 g, b; size_t sh; void* s; };
static std::vector<Cfg> stack;
static void* first4 = nullptr;
extern "C" {
void* stub_first_memset4() { return first4; }
void stub_reset() { first4 = nullptr; }
void stub_note(const char* s) { fprintf(out(), "# %s\n", s); fflush(out()); }
void** __hipRegisterFatBinary(const void*) { static void* h[4]; return h; }
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host, char*, const char* name, unsigned, void*, void*, void*, void*, int*) { names[host] = name; }
int __hipPushCallConfiguration(dim3 g, dim3 b, size_t sh, void* s) { stack.push_back({g, b, sh, s}); return 0; }
int __hipPopCallConfiguration(dim3* g, dim3* b, size_t* sh, void** s) { Cfg c = stack.back(); stack.pop_back(); *g = c.g; *b = c.b; *sh = c.sh; *s = c.s; return 0; }
int hipLaunchKernel(const void* f, dim3 g, dim3 b, void**, size_t sh, void* s) {
  fprintf(out(), "launch %s grid %u %u %u block %u %u %u lds %zu stream %d\n", names.count(f) ? names[f].c_str() : "?", g.x, g.y, g.z, b.x, b.y, b.z, sh, id_of(s));
  return 0;
}
int hipMalloc(void** p, size_t n) { *p = aligned_alloc(256, (n + 255) / 256 * 256); memset(*p, 0, n); return 0; }
int hipFree(void* p) { free(p); return 0; }
int hipMemcpy(void* d, const void* s, size_t n, int k) { memcpy(d, s, n); fprintf(out(), "memcpy %zu kind %d\n", n, k); return 0; }
int hipMemcpyAsync(void* d, const void* s, size_t n, int k, void* st) { memmove(d, s, n); fprintf(out(), "memcpyAsync %zu kind %d stream %d\n", n, k, id_of(st)); return 0; }
int hipMemset(void* d, int v, size_t n) { memset(d, v, n); fprintf(out(), "memset %zu\n", n); return 0; }
int hipMemsetAsync(void* d, int v, size_t n, void* st) { if (n == 4 && !first4) first4 = d; memset(d, v, n); fprintf(out(), "memsetAsync %zu stream %d\n", n, id_of(st)); return 0; }
int hipEventCreate(void** e) { *e = malloc(8); fprintf(out(), "eventCreate\n"); return 0; }
int hipEventCreateWithFlags(void** e, unsigned fl) { *e = malloc(8); fprintf(out(), "eventCreateWithFlags %u\n", fl); return 0; }
int hipEventDestroy(void* e) { fprintf(out(), "eventDestroy\n"); free(e); return 0; }
int hipEventElapsedTime(float* ms, void*, void*) { *ms = 0.f; return 0; }
int hipEventRecord(void* e, void* s) { fprintf(out(), "eventRecord stream %d\n", id_of(s)); return 0; }
int hipEventSynchronize(void*) { return 0; }
int hipFuncSetAttribute(const void* f, int a, int v) { fprintf(out(), "funcSetAttribute %s %d %d\n", names.count(f) ? names[f].c_str() : "?", a, v); return 0; }
const char* hipGetErrorString(int) { return "stub"; }
int hipGetLastError() { return 0; }
int hipStreamCreateWithFlags(void** s, unsigned fl) { *s = malloc(8); fprintf(out(), "streamCreate %u -> %d\n", fl, id_of(*s)); return 0; }
int hipStreamDestroy(void* s) { fprintf(out(), "streamDestroy %d\n", id_of(s)); return 0; }
int hipStreamSynchronize(void* s) { fprintf(out(), "streamSync %d\n", id_of(s)); return 0; }
int hipStreamWaitEvent(void* s, void* e, unsigned) { fprintf(out(), "streamWaitEvent stream %d\n", id_of(s)); return 0; }
}
