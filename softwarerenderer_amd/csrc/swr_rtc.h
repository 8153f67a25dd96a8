// swr_rtc.h -- user programs: the run-time compiler behind swr_program_create / _validate and swr_post_create / _validate.  Included by
// swr_api.hip only, after swr_host.h.
#pragma once

namespace {
// hiprtc is opened with dlopen on first use, not linked: a machine without it loads this library as before, and the program entry
// points answer SWR_ERR_UNSUPPORTED.
struct RtcLib {
    bool ok = false;
    std::string why;
    decltype(&hiprtcCreateProgram) create = nullptr;
    decltype(&hiprtcDestroyProgram) destroy = nullptr;
    decltype(&hiprtcAddNameExpression) add_name = nullptr;
    decltype(&hiprtcCompileProgram) compile = nullptr;
    decltype(&hiprtcGetLoweredName) lowered = nullptr;
    decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
    decltype(&hiprtcGetProgramLog) log = nullptr;
    decltype(&hiprtcGetCodeSize) code_size = nullptr;
    decltype(&hiprtcGetCode) code = nullptr;
};
const RtcLib& rtc_lib() {
    static const RtcLib lib = [] {
        RtcLib r;
#if !defined(SWR_RTC_FLAGS)
        r.why = "this build carries no kernel sources for run-time compilation (built without the Makefile's SWR_RTC_FLAGS)";
        return r;
#else
        std::vector<std::string> names = { "libhiprtc.so", "libhiprtc.so.7" };
        if (const char* rp = getenv("ROCM_PATH")) names.push_back(std::string(rp) + "/lib/libhiprtc.so");
        names.push_back("/opt/rocm/lib/libhiprtc.so");
        void* h = nullptr;
        for (auto& n : names) if ((h = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL))) break;
        if (!h) { r.why = "the HIP run-time compiler (libhiprtc.so) cannot be loaded"; return r; }
        bool all = true;
        auto sym = [&](auto& fp, const char* name) { fp = reinterpret_cast<std::remove_reference_t<decltype(fp)>>(dlsym(h, name)); all = all && fp; };
        sym(r.create, "hiprtcCreateProgram"); sym(r.destroy, "hiprtcDestroyProgram"); sym(r.add_name, "hiprtcAddNameExpression");
        sym(r.compile, "hiprtcCompileProgram"); sym(r.lowered, "hiprtcGetLoweredName"); sym(r.log_size, "hiprtcGetProgramLogSize");
        sym(r.log, "hiprtcGetProgramLog"); sym(r.code_size, "hiprtcGetCodeSize"); sym(r.code, "hiprtcGetCode");
        if (!all) { r.why = "libhiprtc.so lacks an entry point this library needs"; return r; }
        r.ok = true;
        return r;
#endif
    }();
    return lib;
}

// code object + mangled names, in the order of the unit's name expressions: k_raster_c<SWR_PROG_CUSTOM> [EARLYOUT], then (vertex half
// only) k_vertex_user and k_setup; for a post program its k_post instantiations by PostKernel
struct RtcCode { std::vector<char> code; std::vector<std::string> names; bool has_vertex = false; };

// one translation unit for the run-time compiler: what rtc_compile and rtc_compile_post hand to rtc_build
struct RtcUnit {
    std::string key;                     // the in-process cache's key
    std::string src;                     // prelude include, the user's text under its own file name, the kernels
    std::vector<std::string> defines;    // on top of the Makefile's switches and this build's numerics model
    std::vector<std::string> exprs;      // the kernels to look up
    bool has_vertex = false;
};

// Compiles a unit into a gfx950 code object: SWR_OK, SWR_ERR_INVALID_ARG (log = the compiler's messages) or SWR_ERR_UNSUPPORTED.
// In-process cache keyed by the unit's key (the switches are this library's own).
int rtc_build(const RtcUnit& u, std::shared_ptr<const RtcCode>& out, std::string& log) {
    const RtcLib& R = rtc_lib();
    if (!R.ok) { log = R.why; return SWR_ERR_UNSUPPORTED; }
#if defined(SWR_RTC_FLAGS)
    static std::mutex mu;
    static std::map<std::string, std::shared_ptr<const RtcCode>> cache;
    {
        std::lock_guard<std::mutex> g(mu);
        auto it = cache.find(u.key);
        if (it != cache.end()) { out = it->second; return SWR_OK; }
    }
    // the Makefile's code-generation switches and this build's System.Numerics model
    std::vector<std::string> opts;
    {
        const std::string f = SWR_RTC_FLAGS;
        size_t i = 0;
        while (i < f.size()) {
            const size_t j = f.find(' ', i);
            const std::string o = f.substr(i, j == std::string::npos ? std::string::npos : j - i);
            if (!o.empty()) opts.push_back(o);
            if (j == std::string::npos) break;
            i = j + 1;
        }
    }
    opts.push_back("-DSWR_NUMERICS_FMA=" SWR_STR(SWR_NUMERICS_FMA));
    opts.push_back("-DSWR_DOT_PAIRWISE=" SWR_STR(SWR_DOT_PAIRWISE));
    for (auto& d : u.defines) opts.push_back(d);
    std::vector<const char*> copts;
    for (auto& o : opts) copts.push_back(o.c_str());
    const int n_expr = (int)u.exprs.size();
    hiprtcProgram prog = nullptr;
    if (R.create(&prog, u.src.c_str(), "swr_user_program.hip", k_rtc_n_headers, k_rtc_headers, k_rtc_header_names) != HIPRTC_SUCCESS) {
        log = "hiprtcCreateProgram failed";
        return SWR_ERR_UNSUPPORTED;
    }
    for (int k = 0; k < n_expr; ++k) R.add_name(prog, u.exprs[k].c_str());
    const hiprtcResult cr = R.compile(prog, (int)copts.size(), copts.data());
    size_t ls = 0;
    log.clear();
    if (R.log_size(prog, &ls) == HIPRTC_SUCCESS && ls > 1) {
        log.resize(ls);
        if (R.log(prog, &log[0]) != HIPRTC_SUCCESS) log.clear();
        while (!log.empty() && log.back() == '\0') log.pop_back();
    }
    auto code = std::make_shared<RtcCode>();
    bool ok = cr == HIPRTC_SUCCESS;
    code->has_vertex = u.has_vertex;
    code->names.resize(n_expr);
    for (int k = 0; ok && k < n_expr; ++k) {
        const char* mangled = nullptr;
        ok = R.lowered(prog, u.exprs[k].c_str(), &mangled) == HIPRTC_SUCCESS && mangled;
        if (ok) code->names[k] = mangled;
    }
    size_t cs = 0;
    ok = ok && R.code_size(prog, &cs) == HIPRTC_SUCCESS && cs > 0;
    if (ok) { code->code.resize(cs); ok = R.code(prog, code->code.data()) == HIPRTC_SUCCESS; }
    R.destroy(&prog);
    if (ok) {
        // tools/custom_program_numbers.py: the code object as compiled, for its resource usage (never set in production)
        if (const char* dir = getenv("SWR_PROGRAM_DUMP_DIR")) {
            const std::string path = std::string(dir) + "/swr_user_program_" + std::to_string(std::hash<std::string>()(u.key)) + ".co";
            if (FILE* f = fopen(path.c_str(), "wb")) { fwrite(code->code.data(), 1, code->code.size(), f); fclose(f); }
        }
    }
    if (!ok) {
        if (log.empty()) log = "the program did not compile";
        return SWR_ERR_INVALID_ARG;
    }
    std::lock_guard<std::mutex> g(mu);
    out = cache.emplace(u.key, std::shared_ptr<const RtcCode>(code)).first->second;
    return SWR_OK;
#else
    (void)u; (void)out;
    return SWR_ERR_UNSUPPORTED;
#endif
}

// A user program (vertex_src null: the fragment half alone, over the built-in vertex stage).  The compiler's messages name the half as
// vertex.hip:LINE: / fragment.hip:LINE:.  Cached by both texts.
int rtc_compile(const char* vertex_src, const char* user_src, std::shared_ptr<const RtcCode>& out, std::string& log) {
    if (vertex_src && !strstr(vertex_src, "swr_vertex")) {
        if (!rtc_lib().ok) { log = rtc_lib().why; return SWR_ERR_UNSUPPORTED; }
        log = "vertex.hip: the vertex program must define `__device__ void swr_vertex(const swr_vs_in& in, const swr_vs_env& env, swr_vs_out& out)`";
        return SWR_ERR_INVALID_ARG;
    }
    RtcUnit u;
    // (a fragment-only program's key is its text, so `create(fs)` and `create_vf(NULL, fs)` share an entry; '\1' cannot occur in either half's C++)
    u.key = vertex_src ? std::string(vertex_src) + '\1' + user_src : std::string(user_src);
    // prelude (contract + helpers), the user's text under its own file name, then the kernel
    // (with a vertex half: its text first, and behind the raster kernel the geometry header, which under SWR_USER_VERTEX defines
    // k_vertex_user instead of k_vertex and a k_setup that carries data4.w through the clipper)
    u.src = std::string("#include \"swr_program.hip.h\"\n") +
            (vertex_src ? std::string("#line 1 \"vertex.hip\"\n") + vertex_src + "\n" : std::string()) +
            "#line 1 \"fragment.hip\"\n" + user_src +
            "\n#line 1 \"swr_program_kernel\"\n#include \"swr_raster_c.hip.h\"\n" +
            (vertex_src ? "#include \"swr_geometry.hip.h\"\n" : "");
    // the fenced LDS hand-offs (the unfenced ones are verified per (hipcc, source) pair only, DESIGN.md section 8: a run-time compiled
    // kernel is not that pair)
    u.defines = { "-DSWR_RTC_PROGRAM=1", "-DSWR_WAVE_LDS_FENCE=1" };
    if (vertex_src) u.defines.push_back("-DSWR_USER_VERTEX=1");
    u.exprs = { "swr::k_raster_c<false, true, " SWR_STR(SWR_PROG_CUSTOM) ", -1, -1, false>",
                "swr::k_raster_c<false, true, " SWR_STR(SWR_PROG_CUSTOM) ", -1, -1, true>" };
    if (vertex_src) { u.exprs.push_back("swr::k_vertex_user"); u.exprs.push_back("swr::k_setup"); }
    u.has_vertex = vertex_src != nullptr;
    return rtc_build(u, out, log);
}

// A post-process program (swr_post_create / swr_post_validate): the contract and k_post of swr_post.hip.h in front of the user's text,
// whose lines the compiler's messages name as post.hip:LINE:.  k_post has no LDS: neither SWR_RTC_PROGRAM nor the fences apply.
int rtc_compile_post(const char* user_src, std::shared_ptr<const RtcCode>& out, std::string& log) {
    if (!strstr(user_src, "swr_post")) {
        if (!rtc_lib().ok) { log = rtc_lib().why; return SWR_ERR_UNSUPPORTED; }
        log = "post.hip: the post program must define `__device__ float4 swr_post(const swr_post_in& in, const swr_post_env& env)`";
        return SWR_ERR_INVALID_ARG;
    }
    RtcUnit u;
    u.key = std::string("\2") + user_src;           // ('\2' cannot open a fragment or vertex text)
    u.src = std::string("#include \"swr_post.hip.h\"\n#line 1 \"post.hip\"\n") + user_src + "\n";
    u.defines = { "-DSWR_RTC_POST=1" };
    for (const int format : POST_KERNEL_FORMAT) u.exprs.push_back("swr::k_post<" + std::to_string(format) + ">");
    return rtc_build(u, out, log);
}
}  // namespace
