// options.hip -- dgr_set_option / dgr_get_option, the per-thread overrides and the options word, as loops over the table of
// options.h; the initial values from the environment.
#include <cstdlib>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "host_util.h"
#include "kernels.h"
#include "options.h"

namespace dgr {
namespace {

struct OptionDesc {
    const char* name;
    const char* env;
    int def, lo, hi;
    Outside outside;
    int shift;             // field of the options word, or -1
    const char* accepted;  // OUT_REFUSE: the accepted values, in words
};
#define DGR_OPTION_DESC(id, name, env, def, lo, hi, outside, shift, accepted) {name, env, def, lo, hi, outside, shift, accepted},
const OptionDesc k_options[OPT_COUNT] = {DGR_OPTIONS(DGR_OPTION_DESC)};
#undef DGR_OPTION_DESC

// An older name of an option's values 0 / `on` (set: value ? on : 0; get: value == on), with a variable of its own that counts
// only where the option's own variable is unset or not accepted.
struct OptionAlias {
    const char* name;
    const char* env;
    Option of;
    int on;
};
const OptionAlias k_aliases[] = {{"fast_alpha", "DGR_FAST_ALPHA", OPT_ALPHA_MODE, 1}};

constexpr bool fields_fit() {
    for (int i = 0; i < OPT_COUNT; i++)
        if (k_option_shift[i] >= 0 && (k_option_shift[i] % 4 != 0 || k_option_shift[i] / 4 >= DGR_OPT_FIELDS)) return false;
    return true;
}
static_assert(fields_fit(), "an option's field must be one of the DGR_OPT_FIELDS 4-bit fields of the options word");

// What a caller's value becomes; false = refused.
bool accept(const OptionDesc& d, int value, int& out) {
    const bool inside = value >= d.lo && value <= d.hi;
    switch (d.outside) {
        case OUT_CLAMP: out = value < d.lo ? d.lo : value > d.hi ? d.hi : value; return true;
        case OUT_TRUTH: out = value ? 1 : 0; return true;
        case OUT_OFF: out = inside ? value : 0; return true;
        case OUT_REFUSE: out = value; return inside;
    }
    return false;
}

// The one parser of the environment: the whole string is one digit inside the option's range; anything else is ignored.
bool env_digit(const char* variable, int lo, int hi, int& out) {
    const char* e = variable ? getenv(variable) : nullptr;
    if (!e || e[0] < '0' || e[0] > '9' || e[1] != 0 || e[0] - '0' < lo || e[0] - '0' > hi) return false;
    out = e[0] - '0';
    return true;
}
int initial_value(Option o) {
    const OptionDesc& d = k_options[o];
    int v = d.def;
    if (env_digit(d.env, d.lo, d.hi, v)) return v;
    for (const OptionAlias& a : k_aliases)
        if (a.of == o && env_digit(a.env, 0, 1, v)) return v ? a.on : 0;
    return d.def;
}

struct Named {
    int option = -1;  // index into k_options, or -1: no such name
    const OptionAlias* alias = nullptr;
};
Named find(const char* name) {
    const std::string n(name ? name : "");
    Named r;
    for (int i = 0; i < OPT_COUNT; i++)
        if (n == k_options[i].name) r.option = i;
    for (const OptionAlias& a : k_aliases)
        if (n == a.name) { r.option = a.of; r.alias = &a; }
    return r;
}
int refuse(const std::string& text) {
    set_last_error(text);
    return DGR_ERR_BAD_ARGUMENT;
}
std::string range_list(const OptionDesc& d) {
    std::string s;
    for (int v = d.lo; v <= d.hi; v++) s += (v > d.lo ? ", " : "") + std::to_string(v);
    return s;
}

}  // namespace

#define DGR_OPTION_INIT(id, name, env, def, lo, hi, outside, shift, accepted) {initial_value(OPT_##id)},
std::atomic<int> g_option_value[OPT_COUNT] = {DGR_OPTIONS(DGR_OPTION_INIT)};
#undef DGR_OPTION_INIT
__thread int t_option_field[DGR_OPT_FIELDS] = {};

// "blend_wgs_per_cu" as the blend launches see it (kernels.h: launch_blend): the unused dynamic LDS that pads a workgroup
size_t blend_pad_bytes(const void* kernel) {
    const int n = option(OPT_BLEND_WGS_PER_CU);
    if (n < 3 || n > 7) return 0;
    static std::mutex mu;
    static std::vector<std::pair<const void*, size_t>> known;  // static LDS bytes of the blend kernels seen so far
    size_t static_lds = ~(size_t)0;
    {
        std::lock_guard<std::mutex> lk(mu);
        for (const auto& e : known)
            if (e.first == kernel) static_lds = e.second;
        if (static_lds == ~(size_t)0) {
            hipFuncAttributes attr{};
            if (hipFuncGetAttributes(&attr, kernel) != hipSuccess) return 0;
            static_lds = attr.sharedSizeBytes;
            known.emplace_back(kernel, static_lds);
        }
    }
    // the smallest LDS claim that keeps workgroup n + 1 off a CU: n claims then leave the rest of the 160 KB to whatever else
    // fits beside them (160 / n each, as through round 6, left nothing -- and every front-end kernel stages through LDS)
    const size_t per = (((size_t)(160 * 1024) / (size_t)(n + 1)) & ~(size_t)255) + 256;
    return per > static_lds ? per - static_lds : 0;
}

}  // namespace dgr

using namespace dgr;

extern "C" {

int dgr_set_option(const char* name, int value) {
    const Named n = find(name);
    if (n.option < 0) return refuse(std::string("unknown option: ") + (name ? name : ""));
    const OptionDesc& d = k_options[n.option];
    int v = 0;
    if (n.alias) v = value ? n.alias->on : 0;
    else if (!accept(d, value, v)) return refuse(std::string(d.name) + ": " + d.accepted);
    g_option_value[n.option].store(v);
    return DGR_OK;
}
int dgr_get_option(const char* name) {
    const Named n = find(name);
    if (n.option < 0) return DGR_ERR_BAD_ARGUMENT;
    const int v = g_option_value[n.option].load();
    return n.alias ? (v == n.alias->on ? 1 : 0) : v;
}

int dgr_set_thread_option(const char* name, int value) {
    const Named n = find(name);
    if (n.option < 0 || k_options[n.option].shift < 0) return refuse(std::string("not a per-thread option: ") + (name ? name : ""));
    const OptionDesc& d = k_options[n.option];
    int v = -1;  // (< 0: inherit)
    if (value >= 0) {
        if (n.alias) v = value ? n.alias->on : 0;
        else if (!accept(d, value, v)) return refuse(std::string(d.name) + ": " + range_list(d) + " (or < 0: the process-wide option)");
    }
    t_option_field[d.shift / 4] = v + 1;
    return DGR_OK;
}
int dgr_get_thread_option(const char* name) {
    const Named n = find(name);
    if (n.option < 0 || k_options[n.option].shift < 0) return DGR_ERR_BAD_ARGUMENT;
    const int v = thread_option((Option)n.option);
    return n.alias ? (v == n.alias->on ? 1 : 0) : v;
}
// the per-thread options as one word, each field = value + 1 (0 = "inherit", in an override word): DGR_OPT_SHIFT_* in dgr_hip.h
int dgr_thread_options_effective(void) {
    int word = 0;
    for (int i = 0; i < OPT_COUNT; i++)
        if (k_options[i].shift >= 0) word |= (thread_option((Option)i) + 1) << k_options[i].shift;
    return word;
}
int dgr_thread_options_swap(int word) {
    int prev = 0;
    for (int f = 0; f < DGR_OPT_FIELDS; f++) {
        prev |= t_option_field[f] << (4 * f);
        if (word >= 0) t_option_field[f] = (word >> (4 * f)) & 15;
    }
    return prev;
}

}  // extern "C"
