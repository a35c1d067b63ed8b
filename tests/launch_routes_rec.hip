// Launch recorder of tests/test_launch_routes_cpu.py: gemm.hip or attention.hip as they are, in a host-only build
// (hipcc --offload-host-only -std=c++17 -I mcm_amd/csrc -DREC_GEMM | -DREC_ATTN), with every kernel launch replaced by
// a line on stdout and the device query by a CU count from argv.  It runs nothing and needs no GPU.
//
// usage: rec CUS < cases
//   G prec epi M N K ldx ldo ksplit xsplit px hm    launch_gemm of that problem (px: 1 = a pixel source is set)
//   Q prec epi M N                                  gemm_fold_kind, gemm_ln_tail_ok, gemm_patch_takes_pixels, grid
//   T prec nseq L heads head_dim causal qrows reverse hm split      launch_attention
//   V n / O n / A n                                 harness builds: gemm variant, grid override, attention variant
// A case prints itself, one line per launch it made, and its hipError_t.
#include <hip/hip_runtime.h>

#include <cxxabi.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <typeinfo>

struct GemmArgs;
namespace rec_detail {
int g_cus = 0;
const char* g_base[3] = {nullptr, nullptr, nullptr};  // x, out, resid of the case being run
template <auto K> struct Tag {};
template <auto K> std::string kernel_name() {  // the instantiation with its template arguments
  int st = 0;
  char* d = abi::__cxa_demangle(typeid(Tag<K>).name(), nullptr, nullptr, &st);
  std::string n = st == 0 && d ? d : typeid(Tag<K>).name();
  free(d);
  const std::string pre = "rec_detail::Tag<", anon = "(anonymous namespace)::";
  if (n.compare(0, pre.size(), pre) == 0) n = n.substr(pre.size(), n.size() - pre.size() - 1);
  for (size_t p; (p = n.find(anon)) != std::string::npos;) n.erase(p, anon.size());
  while (!n.empty() && (n[0] == '&' || n[0] == '(')) n.erase(0, 1);
  const size_t sig = n.rfind(">(");  // "(parameter types)" of a function-pointer argument, when the demangler prints them
  if (sig != std::string::npos) n.erase(sig + 1);
  if (n.compare(0, 5, "void ") == 0) n.erase(0, 5);
  return n;
}
template <class G> void print_gemm(const G& a);  // defined once GemmArgs is complete
template <class T> void print_arg(const T& v) {
  using U = std::decay_t<T>;
  if constexpr (std::is_same_v<U, GemmArgs>) print_gemm(v);
  else if constexpr (std::is_integral_v<U>) printf(" %lld", (long long)v);
  else if constexpr (std::is_pointer_v<U>) printf(" %c", v ? 'p' : '0');
}
template <auto K, class... A> void rec(dim3 g, dim3 b, int lds, const A&... args) {
  printf("  %s grid=%u,%u,%u block=%u lds=%d |", kernel_name<K>().c_str(), g.x, g.y, g.z, b.x, lds);
  (print_arg(args), ...);
  printf("\n");
}
inline hipError_t get_device(int* d) { *d = 0; return hipSuccess; }
inline hipError_t device_attr(int* v, hipDeviceAttribute_t, int) { *v = g_cus; return hipSuccess; }
}  // namespace rec_detail

#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(k, g, b, l, s, ...) rec_detail::rec<k>(g, b, (int)(l), __VA_ARGS__)
#define hipFuncSetAttribute(...) hipSuccess
#define hipGetLastError() hipSuccess
#define hipGetDevice(d) rec_detail::get_device(d)
#define hipDeviceGetAttribute(v, a, d) rec_detail::device_attr(v, a, d)

#if defined(REC_GEMM)
#include "gemm.hip"
#elif defined(REC_ATTN)
#include "attention.hip"
#else
#error "build with -DREC_GEMM or -DREC_ATTN"
#endif

template <class G> void rec_detail::print_gemm(const G& a) {
  printf(" M=%d N=%d K=%d gn=%d x+%lld out+%lld resid+%lld", a.M, a.N, a.K, a.gn, (long long)((const char*)a.x - g_base[0]),
         a.out ? (long long)((const char*)a.out - g_base[1]) : -1LL, a.resid ? (long long)((const char*)a.resid - g_base[2]) : -1LL);
}

int main(int argc, char** argv) {
  rec_detail::g_cus = argc > 1 ? atoi(argv[1]) : 256;
  static char x[16], out[16], resid[16], other[16];  // distinct bases; nothing is ever dereferenced
  char line[512];
  while (fgets(line, sizeof line, stdin)) {
    line[strcspn(line, "\n")] = 0;
    long long v[12] = {};
    const int n = sscanf(line + 1, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", v, v + 1, v + 2, v + 3, v + 4,
                         v + 5, v + 6, v + 7, v + 8, v + 9, v + 10, v + 11);
    printf("%s\n", line);
    hipError_t e = hipSuccess;
    switch (line[0]) {
#ifdef REC_GEMM
      case 'G': {
        if (n != 11) return 2;
        const int epi = (int)v[1];
        GemmArgs a{};
        a.x = x; a.w = other; a.bias = (const float*)other;
        if (epi == EPI_RESID) a.resid = (float*)resid; else a.out = out;
        if (epi == EPI_PATCH) { a.pos = (const float*)other; a.np = 49; a.img = 224; a.patch = 32; }
        a.M = (int)v[2]; a.N = (int)v[3]; a.K = (int)v[4]; a.ldx = (int)v[5]; a.ldo = (int)v[6];
        a.ksplit = (int)v[7]; a.xsplit = (int)v[8];
        if (v[9]) a.px = (const float*)other;
        a.hm = (int)v[10];
        rec_detail::g_base[0] = x; rec_detail::g_base[1] = out; rec_detail::g_base[2] = resid;
        e = launch_gemm((int)v[0], epi, a, nullptr);
        break;
      }
      case 'Q':
        if (n != 4) return 2;
        printf("  fold_kind=%d ln_tail_ok=%d patch_takes_pixels=%d grid=%d\n", gemm_fold_kind((int)v[1], (int)v[2], (int)v[3]),
               (int)gemm_ln_tail_ok((int)v[0], (int)v[2], (int)v[3]),
               (int)gemm_patch_takes_pixels((int)v[0], (int)v[2], (int)v[3], 3 * 32 * 32, 32, 224), gemm_persistent_grid());
        break;
#ifdef MCM_HARNESS
      case 'V': gemm_set_variant((int)v[0]); break;
      case 'O': gemm_set_persistent_grid((int)v[0]); break;
#endif
#endif
#ifdef REC_ATTN
      case 'T':
        if (n != 10) return 2;
        e = launch_attention((int)v[0], x, out, (int)v[1], (int)v[2], (int)v[3], (int)v[4], v[5] != 0, (int)v[6], nullptr, v[7] != 0,
                             (int)v[8], v[9] != 0, nullptr);
        break;
#ifdef MCM_HARNESS
      case 'A': attention_set_variant((int)v[0]); break;
#endif
#endif
      default: return 2;
    }
    printf("  -> %d\n", (int)e);
  }
  return 0;
}
