// pybind11 module `kfunca_amd._C`: the Python surface of the reference's `kfunca` module
// (src/register.cpp:59-225) — same function names, arities and semantics — over the rebuilt host core.
// kfunca_amd/__init__.py re-exports it, so `import kfunca_amd as kfunca` runs the reference's tests.
#include <pybind11/numpy.h>
#include <cstdlib>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <iostream>
#include <vector>

#include "allocator.h"
#include "attn_full.h"
#include "comm.h"
#include "device_api.h"
#include "expert_linear.h"
#include "fp8.h"
#include "glu.h"
#include "linear_ce.h"
#include "moe.h"
#include "softmax.h"
#include "ops.h"
#include "optim.h"
#include "qk_norm.h"
#include "rope.h"
#include "tensor.h"
#include "tensor_iterator.h"

namespace py = pybind11;

namespace {

struct NpType { char kind; int size; ScalarType st; };
const NpType kNpTypes[] = {{'b', 1, ScalarType::Bool}, {'u', 1, ScalarType::Byte}, {'i', 1, ScalarType::Char},
                           {'i', 2, ScalarType::Short}, {'i', 4, ScalarType::Int}, {'i', 8, ScalarType::Long},
                           {'f', 2, ScalarType::Half}, {'f', 4, ScalarType::Float}, {'f', 8, ScalarType::Double}};

Tensor from_numpy(py::array array, int device) {
    const char kind = array.dtype().kind();
    const int size = (int)array.dtype().itemsize();
    for (const auto &t : kNpTypes) {
        if (t.kind != kind || t.size != size) continue;
        py::array c = py::array::ensure(array, py::array::c_style); // the reference ignores strides (register.cpp:27-39); we honour them
        std::vector<int64_t> shape(c.shape(), c.shape() + c.ndim());
        Tensor out = empty(shape, t.st, device);
        if (out.numel() > 0) out.copy_from_cpu_ptr(const_cast<void *>(c.data()));
        return out;
    }
    throw std::runtime_error("Unsupported dtype in from_numpy()");
}

py::array to_numpy(const Tensor &t) {
    CHECK_FAIL(t.defined());
    CHECK_FAIL(t.is_dense()); // (the reference asks its flag, register.cpp:42: it refuses dense views too)
    const char *np = nullptr;
    switch (t.dtype()) {
    case ScalarType::Bool: np = "bool"; break;
    case ScalarType::Byte: np = "uint8"; break;
    case ScalarType::Char: np = "int8"; break;
    case ScalarType::Short: np = "int16"; break;
    case ScalarType::Int: np = "int32"; break;
    case ScalarType::Long: np = "int64"; break;
    case ScalarType::Half: np = "float16"; break;
    case ScalarType::Float: np = "float32"; break;
    case ScalarType::Double: np = "float64"; break;
    // numpy has no bfloat16: the raw bits come back as uint16 (x.view(np.uint32) << 16 is the f32 value; ml_dtypes users can
    // .view(ml_dtypes.bfloat16)). The reference's to_numpy rejects half and bfloat16 altogether (register.cpp:41-57).
    case ScalarType::BFloat16: np = "uint16"; break;
    default: throw std::runtime_error("Unsupported dtype in to_numpy()");
    }
    py::array out(py::dtype(np), t.sizes());
    // a contiguous view may sit inside a larger storage: copy exactly numel elements from data_ptr()
    const size_t bytes = (size_t)t.numel() * (size_t)t.element_size_in_bytes();
    if (bytes) DEV_CALL(kf_memcpy_d2h(out.mutable_data(), t.data_ptr(), bytes, dev::stream(t.device())));
    return out;
}

std::vector<int64_t> args_to_dims(const py::args &args) {
    std::vector<int64_t> dims;
    for (auto a : args) dims.push_back(a.cast<int64_t>());
    return dims;
}

Tensor get_item(Tensor &self, py::object key) {
    Tensor out = self;
    auto apply = [&](py::handle item, int &dim) {
        if (py::isinstance<py::slice>(item)) {
            size_t start, stop, step, len;
            if (!item.cast<py::slice>().compute(out.shape(dim), &start, &stop, &step, &len)) throw py::error_already_set();
            out = out.slice(dim, (int64_t)start, (int64_t)stop, (int64_t)step);
            ++dim;
        } else if (py::isinstance<py::int_>(item)) {
            out = out.select(dim, item.cast<int64_t>()); // the selected dim disappears
        } else {
            throw py::type_error("tensor indices must be ints or slices");
        }
    };
    int dim = 0;
    if (py::isinstance<py::tuple>(key)) {
        auto tup = key.cast<py::tuple>();
        CHECK_FAIL((int)tup.size() <= self.dim());
        for (auto item : tup) apply(item, dim);
    } else {
        apply(key, dim);
    }
    return out;
}

// CPU-only window onto the geometry engine: operands are (shape, strides_in_elements, dtype, defined)
py::dict iter_geometry(std::vector<std::tuple<std::vector<int64_t>, std::vector<int64_t>, ScalarType, bool>> outputs,
                       std::vector<std::tuple<std::vector<int64_t>, std::vector<int64_t>, ScalarType, bool>> inputs, bool is_reduction,
                       int64_t reduce_dim, bool resize_outputs, std::vector<int> aliases, bool check_mem_overlap) {
    IterGeometry g;
    std::vector<int> ids(outputs.size() + inputs.size());
    int slot = 0;
    auto add = [&](const auto &spec, bool is_out, int idx) {
        IterOperand op;
        op.defined = std::get<3>(spec);
        const auto &shape = std::get<0>(spec);
        const auto &stride = std::get<1>(spec);
        op.ndim = (int)shape.size();
        for (int d = 0; d < op.ndim; ++d) {
            op.shape[d] = shape[d];
            op.stride[d] = d < (int)stride.size() ? stride[d] : 0;
        }
        op.dtype = std::get<2>(spec);
        op.device = op.defined ? 0 : -1;
        op.data = reinterpret_cast<char *>(0x10000000ull * (uint64_t)(idx + 1));
        int alias = idx < (int)aliases.size() ? aliases[idx] : -1;
        ids[idx] = alias >= 0 ? alias : idx;
        op.identity = reinterpret_cast<const void *>((uintptr_t)(ids[idx] + 1));
        if (alias >= 0) op.data = reinterpret_cast<char *>(0x10000000ull * (uint64_t)(alias + 1));
        g.add(op, is_out);
    };
    for (auto &o : outputs) { add(o, true, slot); ++slot; }
    for (auto &i : inputs) { add(i, false, slot); ++slot; }
    std::vector<std::vector<int64_t>> allocated(outputs.size());
    auto alloc = [&](int arg, const int64_t *shape, int ndim, ScalarType dtype, int device, IterOperand &op) {
        op.defined = true;
        op.ndim = ndim;
        int64_t run = 1;
        for (int d = ndim - 1; d >= 0; --d) {
            op.shape[d] = shape[d];
            op.stride[d] = run;
            run *= shape[d];
        }
        op.dtype = dtype;
        op.device = device;
        op.data = reinterpret_cast<char *>(0x70000000ull + 0x1000000ull * (uint64_t)arg);
        allocated[arg].assign(shape, shape + ndim);
    };
    g.build(is_reduction, reduce_dim, resize_outputs, check_mem_overlap, alloc);
    py::dict r;
    std::vector<int64_t> shape, perm;
    for (int d = 0; d < g.ndim(); ++d) shape.push_back(g.shape(d));
    std::vector<std::vector<int64_t>> strides;
    for (int t = 0; t < g.ntensors(); ++t) {
        std::vector<int64_t> s;
        for (int d = 0; d < g.ndim(); ++d) s.push_back(g.stride_bytes(t, d));
        strides.push_back(s);
    }
    r["ndim"] = g.ndim();
    r["shape"] = shape;
    r["stride_bytes"] = strides;
    r["common_dtype"] = g.common_dtype();
    r["numel"] = g.numel();
    r["num_output_elements"] = g.num_output_elements();
    r["is_contiguous"] = g.is_contiguous();
    r["can_use_32bit_indexing"] = g.can_use_32bit_indexing();
    r["allocated"] = allocated;
    int pieces = 0;
    int64_t covered = 0;
    g.for_each_32bit([&](const IterGeometry &p) { ++pieces; covered += p.numel(); });
    r["pieces_32bit"] = pieces;
    r["pieces_numel"] = covered;
    return r;
}

} // namespace

PYBIND11_MODULE(_C, m) {
    py::register_exception<utils::Error>(m, "Error", PyExc_RuntimeError);

    m.def("device_info", []() {
        const int n = dev::device_count();
        std::cout << "HIP devices: " << n << "\n";
        for (int i = 0; i < n; ++i) {
            kf_device_props p;
            DEV_CALL(kf_device_props_get(i, &p));
            std::cout << "[" << i << "] " << p.name << " (" << p.arch << "), " << p.compute_units << " CUs, wave " << p.wavefront_size
                      << ", " << p.clock_khz / 1000 << " MHz, LDS/block " << p.lds_per_block << " B, L2 " << p.l2_bytes << " B, HBM "
                      << p.total_mem / (1ull << 30) << " GiB (free " << p.free_mem / (1ull << 30) << " GiB)\n";
        }
    });
    m.def("device_count", &dev::device_count);
    m.def("synchronize", [](int device) { dev::synchronize(device); }, py::arg("device") = 0);
    // HIP graphs over the device's stream (extension; the reference launches kernel by kernel, launcher_cuda.h:330-354): record
    // whatever the operator API enqueues between begin and end - a whole forward + backward step - and replay it with one
    // submission. Replays read and write the addresses captured, so the allocator runs in capture mode meanwhile: every block
    // the recorded step allocates or frees stays in a pool private to the graph (never re-enters the shared cache) until
    // graph_destroy - an eager op, a from_numpy or another step between two replays cannot be handed the graph's scratch.
    // Results the caller still holds when the capture ends are rewritten by every replay (that is the point of replaying).
    struct GraphHandle { void *exec; uint64_t pool; int device; };
    static uint64_t open_capture_pool = 0;
    m.def("graph_begin", [](int device) {
        void *st = dev::stream(device);
        open_capture_pool = utils::memory::DeviceAllocator::GetInstance()->begin_capture(device);
        const int rc = kf_graph_begin_capture(st);
        if (rc != KF_OK) {
            utils::memory::DeviceAllocator::GetInstance()->release_graph(open_capture_pool);
            open_capture_pool = 0;
            DEV_CALL(rc);
        }
    }, py::arg("device") = 0);
    m.def("graph_end", [](int device) {
        void *g = nullptr;
        const uint64_t pool = open_capture_pool;
        open_capture_pool = 0;
        const int rc = kf_graph_end_capture(dev::stream(device), &g);
        utils::memory::DeviceAllocator::GetInstance()->end_capture(pool);
        if (rc != KF_OK) {
            utils::memory::DeviceAllocator::GetInstance()->release_graph(pool);
            DEV_CALL(rc);
        }
        return reinterpret_cast<uintptr_t>(new GraphHandle{g, pool, device});
    }, py::arg("device") = 0);
    m.def("graph_launch", [](uintptr_t g, int device) {
        auto *h = reinterpret_cast<GraphHandle *>(g);
        CHECK_FAIL(h && h->exec, "graph_launch: null graph");
        DEV_CALL(kf_graph_launch(h->exec, dev::stream(device)));
    }, py::arg("graph"), py::arg("device") = 0);
    m.def("graph_destroy", [](uintptr_t g) {
        auto *h = reinterpret_cast<GraphHandle *>(g);
        if (!h) return;
        dev::synchronize(h->device); // no replay may still be running when its scratch goes back to the shared cache
        DEV_CALL(kf_graph_destroy(h->exec));
        utils::memory::DeviceAllocator::GetInstance()->release_graph(h->pool);
        delete h;
    });
    m.def("memstat", []() { utils::memory::DeviceAllocator::GetInstance()->print(); });
    m.def("memstat_dict", [](int device) {
        auto s = utils::memory::DeviceAllocator::GetInstance()->stats(device);
        py::dict d;
        d["active_blocks"] = s.active_blocks;
        d["cached_blocks"] = s.cached_blocks;
        d["active_bytes"] = s.active_bytes;
        d["cached_bytes"] = s.cached_bytes;
        d["driver_allocs"] = s.driver_allocs;
        d["graph_blocks"] = s.graph_blocks;
        d["graph_bytes"] = s.graph_bytes;
        return d;
    }, py::arg("device") = -1);

    py::enum_<ScalarType>(m, "dtype", py::module_local()) // module-local: the reference's own module (oracle/_ref) binds the same C++ names
        .value("byte", ScalarType::Byte)
        .value("char", ScalarType::Char)
        .value("short", ScalarType::Short)
        .value("int", ScalarType::Int)
        .value("long", ScalarType::Long)
        .value("half", ScalarType::Half)
        .value("bfloat16", ScalarType::BFloat16)
        .value("float", ScalarType::Float)
        .value("double", ScalarType::Double)
        .value("bool", ScalarType::Bool)
        .export_values();

    m.def("empty", [](std::vector<int64_t> shape, ScalarType dtype, int device) { return empty(shape, dtype, device); });
    m.def("empty_like", [](const Tensor &self) { return empty_like(self); });
    m.def("from_numpy", &from_numpy);
    m.def("to_numpy", &to_numpy);
    m.def("zeros", [](std::vector<int64_t> shape, ScalarType dtype, int device) { return zeros(shape, dtype, device); });
    m.def("causal_attention", &gpu::causal_attention);
    // the reference's roadmap operators (README.md:28-30)
    // ---- collectives (extension: the reference has no distributed code): one process per GPU, one RCCL communicator
    // per process through the C ABI; the 128-byte id travels out of band (kfunca_amd.parallel uses torch.distributed / gloo for that)
    m.def("comm_unique_id", []() { return py::bytes(gpu::comm_unique_id()); });
    m.def("comm_init", [](py::bytes id, int rank, int world_size, int device) { gpu::comm_init(std::string(id), rank, world_size, device); },
          py::arg("unique_id"), py::arg("rank"), py::arg("world_size"), py::arg("device") = 0);
    m.def("comm_destroy", &gpu::comm_destroy);
    m.def("comm_initialized", &gpu::comm_initialized);
    m.def("comm_rank", &gpu::comm_rank);
    m.def("comm_world_size", &gpu::comm_world_size);
    m.def("all_reduce_", [](py::object x) { // a tensor, or a list of tensors reduced as ONE collective launch; in place, returns its argument
        if (py::isinstance<py::list>(x) || py::isinstance<py::tuple>(x)) {
            std::vector<Tensor> ts = x.cast<std::vector<Tensor>>();
            gpu::all_reduce_(ts);
        } else {
            Tensor t = x.cast<Tensor>();
            gpu::all_reduce_(t);
        }
        return x;
    });
    // torch.optim.AdamW's constructor: params is a list of tensors or of groups {"params": [...], "weight_decay": wd}
    py::class_<gpu::AdamW, std::shared_ptr<gpu::AdamW>>(m, "AdamW", py::module_local())
        .def(py::init([](py::iterable params, double lr, std::pair<double, double> betas, double eps, double weight_decay, py::object max_grad_norm,
                         double grad_scale, bool master_weights) {
                 std::vector<gpu::AdamW::Group> groups;
                 gpu::AdamW::Group plain{{}, weight_decay};
                 for (py::handle h : params) {
                     if (py::isinstance<py::dict>(h)) {
                         py::dict d = py::reinterpret_borrow<py::dict>(h);
                         gpu::AdamW::Group g{{}, weight_decay};
                         for (auto kv : d) {
                             const std::string key = py::str(kv.first);
                             if (key == "params") {
                                 if (py::isinstance<Tensor>(kv.second)) g.params.push_back(kv.second.cast<Tensor>());
                                 else for (py::handle t : py::reinterpret_borrow<py::iterable>(kv.second)) g.params.push_back(t.cast<Tensor>());
                             } else if (key == "weight_decay") {
                                 g.weight_decay = kv.second.cast<double>();
                             } else {
                                 throw py::value_error("AdamW: parameter group key '" + key + "' is not supported (only 'params' and 'weight_decay')");
                             }
                         }
                         if (!d.contains("params")) throw py::value_error("AdamW: a parameter group needs 'params'");
                         groups.push_back(std::move(g));
                     } else {
                         plain.params.push_back(h.cast<Tensor>());
                     }
                 }
                 if (!plain.params.empty()) {
                     if (!groups.empty()) throw py::value_error("AdamW: params mixes tensors and parameter groups");
                     groups.push_back(std::move(plain));
                 }
                 return std::make_shared<gpu::AdamW>(groups, lr, betas.first, betas.second, eps, max_grad_norm.is_none() ? 0.0 : max_grad_norm.cast<double>(),
                                                     grad_scale, master_weights);
             }),
             py::arg("params"), py::arg("lr") = 1e-3, py::arg("betas") = std::make_pair(0.9, 0.999), py::arg("eps") = 1e-8, py::arg("weight_decay") = 1e-2,
             py::arg("max_grad_norm") = py::none(), py::arg("grad_scale") = 1.0, py::arg("master_weights") = true)
        .def("step", [](gpu::AdamW &o) -> py::object {
            Tensor n = o.step();
            if (!n.defined()) return py::none();
            return py::cast(n);
        })
        .def("zero_grad", &gpu::AdamW::zero_grad)
        .def("set_lr", &gpu::AdamW::set_lr, py::arg("lr"))
        .def_property_readonly("lr", &gpu::AdamW::lr)
        .def("state", [](const gpu::AdamW &o, const Tensor &p) -> py::tuple {
            auto [m, v, s, ms] = o.state(p);
            return py::make_tuple(m, v, s, ms.defined() ? py::cast(ms) : py::none());
        }, py::arg("param"))
        .def("__len__", &gpu::AdamW::size);
    py::class_<gpu::GradBucket, std::shared_ptr<gpu::GradBucket>>(m, "GradBucket", py::module_local())
        .def(py::init([](const std::vector<Tensor> &params, double cap_mb, bool accum_f32) {
                 return gpu::GradBucket::create(params, (int64_t)(cap_mb * 1048576.0), accum_f32);
             }),
             py::arg("params"), py::arg("cap_mb") = 256.0, py::arg("accum_f32") = false)
        .def("attach", &gpu::GradBucket::attach)
        .def("detach", &gpu::GradBucket::detach)
        .def("wait", &gpu::GradBucket::wait)
        .def("flat", &gpu::GradBucket::flat)
        .def("reduced_bytes", &gpu::GradBucket::reduced_bytes)
        .def("set_collectives", &gpu::GradBucket::set_collectives)
        .def("chunk_ms", &gpu::GradBucket::chunk_ms)
        .def("fired_order", [](const gpu::GradBucket &b) { return b.fired_order(); })
        .def("chunks", [](const gpu::GradBucket &b) {
            py::list out;
            for (const auto &c : b.chunks()) out.append(py::make_tuple(c.first, c.last, c.offset, c.numel));
            return out;
        })
        // the layout arithmetic alone (no device): [(first, last, offset, numel)], chunk 0 = the LAST parameters
        .def_static("plan", [](const std::vector<int64_t> &numels, int64_t cap_elements) {
            py::list out;
            for (const auto &c : gpu::GradBucket::plan(numels, cap_elements)) out.append(py::make_tuple(c.first, c.last, c.offset, c.numel));
            return out;
        })
        // the firing bookkeeping alone (no device; the code arrived() / wait() run): chunk indices in the order their collectives leave
        .def_static("simulate_fired_order", &gpu::GradBucket::simulate_fired_order, py::arg("numels"), py::arg("cap_elements"), py::arg("arrivals"));

    m.def("rms_norm", [](const Tensor &x, py::object w, double eps) { return gpu::rms_norm(x, w.is_none() ? Tensor() : w.cast<Tensor>(), eps); },
          py::arg("x"), py::arg("weight") = py::none(), py::arg("eps") = 1e-5);
    m.def("layer_norm", [](const Tensor &x, py::object w, py::object b, double eps) {
        return gpu::layer_norm(x, w.is_none() ? Tensor() : w.cast<Tensor>(), b.is_none() ? Tensor() : b.cast<Tensor>(), eps);
    }, py::arg("x"), py::arg("weight") = py::none(), py::arg("bias") = py::none(), py::arg("eps") = 1e-5);
    m.def("embedding", &gpu::embedding, py::arg("table"), py::arg("indices"));
    // torch's F.cross_entropy argument names; the class axis is the LAST dim of logits
    m.def("cross_entropy", [](const Tensor &logits, const Tensor &target, int64_t ignore_index, const std::string &reduction, double label_smoothing) {
        int r = -1;
        if (reduction == "none") r = KF_CE_NONE;
        else if (reduction == "sum") r = KF_CE_SUM;
        else if (reduction == "mean") r = KF_CE_MEAN;
        CHECK_FAIL(r >= 0, reduction, " is not a valid value for reduction");
        return gpu::cross_entropy(logits, target, ignore_index, r, label_smoothing);
    }, py::arg("logits"), py::arg("target"), py::arg("ignore_index") = -100, py::arg("reduction") = "mean", py::arg("label_smoothing") = 0.0);
    // the LM head and its loss in chunks of chunk_rows tokens, never holding the [T, V] logits; weight is [V, d] (embedding's table layout)
    m.def("linear_cross_entropy", [](const Tensor &x, const Tensor &weight, const Tensor &target, int64_t ignore_index, const std::string &reduction,
                                     double label_smoothing, double z_loss, int64_t chunk_rows) {
        int r = -1;
        if (reduction == "none") r = KF_CE_NONE;
        else if (reduction == "sum") r = KF_CE_SUM;
        else if (reduction == "mean") r = KF_CE_MEAN;
        CHECK_FAIL(r >= 0, reduction, " is not a valid value for reduction");
        return gpu::linear_cross_entropy(x, weight, target, ignore_index, r, label_smoothing, z_loss, chunk_rows);
    }, py::arg("x"), py::arg("weight"), py::arg("target"), py::arg("ignore_index") = -100, py::arg("reduction") = "mean",
          py::arg("label_smoothing") = 0.0, py::arg("z_loss") = 0.0, py::arg("chunk_rows") = 0);
    // NOT part of the operator surface (underscore, not in __all__): a hook for the CPU-only ABI test and tools/linear_ce_bench.py, which
    // reach linear_cross_entropy's chunk_rows check and its default without a device. 0: the default; raises on anything but 0 or a
    // positive multiple of 128.
    m.def("_linear_ce_chunk_rows", &gpu::linear_ce_chunk_rows, py::arg("chunk_rows") = 0);
    // per-tensor scaled FP8 (fp8.h): FP8 codes travel as Byte tensors, the format as "e4m3" / "e5m2"
    auto fp8_fmt = [](const std::string &fmt) {
        CHECK_FAIL(fmt == "e4m3" || fmt == "e5m2", fmt, " is not an FP8 format: e4m3 or e5m2");
        return fmt == "e4m3" ? KF_FP8_E4M3 : KF_FP8_E5M2;
    };
    m.def("fp8_quantize", [fp8_fmt](const Tensor &x, const std::string &fmt, bool transpose) {
        const gpu::Fp8Quantized r = gpu::fp8_quantize(x, fp8_fmt(fmt), transpose);
        return py::make_tuple(r.q, transpose ? py::cast(r.qt) : py::object(py::none()), r.scale_inv);
    }, py::arg("x"), py::arg("fmt") = "e4m3", py::arg("transpose") = false,
          "fp8_quantize(x [..., cols], fmt='e4m3', transpose=False) -> (q, qt or None, scale_inv): q Byte [rows, cols] = the FP8 codes of x * 2^e, "
          "e the largest integer with max|x| * 2^e <= the format's maximum (448 / 57344); qt Byte [cols, ceil16(rows)] = the transposed codes "
          "with zero bytes in the pad columns; scale_inv Float [1] = 2^-e on the device. float, half or bfloat16; x may be row-pitched. "
          "Nothing is read back to the host.");
    m.def("gemm_fp8", [fp8_fmt](const Tensor &a_q, const Tensor &b_q, const Tensor &scale_inv_a, const Tensor &scale_inv_b, const std::string &fmt_a,
                                const std::string &fmt_b, ScalarType out_dtype) {
        return gpu::gemm_fp8(a_q, b_q, scale_inv_a, scale_inv_b, fp8_fmt(fmt_a), fp8_fmt(fmt_b), out_dtype);
    }, py::arg("a_q"), py::arg("b_q"), py::arg("scale_inv_a"), py::arg("scale_inv_b"), py::arg("fmt_a") = "e4m3", py::arg("fmt_b") = "e4m3",
          py::arg("out_dtype") = ScalarType::BFloat16,
          "gemm_fp8(a_q [M, K], b_q [N, K], scale_inv_a, scale_inv_b, fmt_a='e4m3', fmt_b='e4m3', out_dtype=bfloat16) -> [M, N] = "
          "scale_inv_a * scale_inv_b * a_q b_q^T, f32 accumulation on the block-scaled matrix pipe. Byte operands with unit stride along K; K "
          "and the row strides are multiples of 16.");
    m.def("linear_fp8", &gpu::linear_fp8, py::arg("x"), py::arg("weight"),
          "linear_fp8(x [..., K], weight [N, K]) -> [..., N] in x's dtype (float, half, bfloat16): both operands quantised to e4m3 with "
          "per-tensor power-of-two scales. Differentiable in x and weight: the backward quantises dy to e5m2 and keeps only the transposed FP8 "
          "copies of x and weight and the two scales. K and N must be multiples of 16. No host synchronisation: forward and backward capture "
          "into a graph.");
    // NOT part of the operator surface: linear_fp8's shape rule without a device, for the CPU-only ABI test
    m.def("_linear_fp8_check_dims", &gpu::linear_fp8_check_dims, py::arg("K"), py::arg("N"));
    m.def("gemm_fused", [](const Tensor &a, const Tensor &b, float alpha, py::object bias, py::object mul, py::object add) {
        auto opt = [](py::object o) { return o.is_none() ? Tensor() : o.cast<Tensor>(); };
        return gpu::gemm_fused(a, b, alpha, opt(bias), opt(mul), opt(add));
    }, py::arg("a"), py::arg("b"), py::arg("alpha") = 1.0f, py::arg("bias") = py::none(), py::arg("mul") = py::none(), py::arg("add") = py::none());
    // the roadmap's name (README.md:32): the fused QKV projection = one GEMM with the bias in its store; its packed [B*S, 3*H*D] output
    // is what causal_attention_qkv reads in place
    m.def("qkv_linear", [](const Tensor &x, const Tensor &w_qkv, py::object bias) {
        return gpu::gemm_fused(x, w_qkv, 1.0f, bias.is_none() ? Tensor() : bias.cast<Tensor>(), Tensor(), Tensor());
    }, py::arg("x"), py::arg("w_qkv"), py::arg("bias") = py::none());
    // kv_heads: grouped-query attention on the packed [B*S, (H + 2*kv_heads)*D] projection (rope_qkv's kv_heads layout)
    m.def("causal_attention_qkv", [](const Tensor &qkv, int64_t B, int64_t S, int64_t H, py::object kv_heads) {
        return gpu::causal_attention_qkv(qkv, B, S, H, kv_heads.is_none() ? -1 : kv_heads.cast<int64_t>());
    }, py::arg("qkv"), py::arg("B"), py::arg("S"), py::arg("H"), py::arg("kv_heads") = py::none());
    m.def("causal_attention_gqa", &gpu::causal_attention_gqa, py::arg("q"), py::arg("k"), py::arg("v"));
    // full (non-causal) attention with an optional per-batch key length (Long [B]): encoder self-attention, cross-attention, padded batches
    // causal = True: the prefix-LM mask (full inside prefix_len[b], causal after it; prefix_len = None: causal over a padded batch)
    // window = (left, right): the sliding-window mask, keys m - left .. m + right of query m; None in a place: unbounded on that side
    auto opt = [](const py::object &t) { return t.is_none() ? Tensor() : t.cast<Tensor>(); };
    auto win = [](const char *op, const py::object &w, gpu::AttentionWindow &out) -> const gpu::AttentionWindow * {
        if (w.is_none()) return nullptr;
        const std::string text = std::string(op) + ": window is a pair (left, right) of non-negative ints, or None for unbounded on that side";
        if (!py::isinstance<py::sequence>(w) || py::len(w) != 2) throw py::value_error(text);
        const py::sequence s = w.cast<py::sequence>();
        int64_t v[2];
        for (int i = 0; i < 2; ++i) {
            const py::object e = s[i];
            if (e.is_none()) { v[i] = -1; continue; }
            if (!py::isinstance<py::int_>(e) || e.cast<int64_t>() < 0) throw py::value_error(text);
            v[i] = e.cast<int64_t>();
        }
        out = {v[0], v[1]};
        return &out;
    };
    // doc_mask = doc_mask(cu_doclens, S): the document mask of packed rows - several sequences end to end in one row, attention inside each
    py::class_<gpu::DocMask>(m, "DocMask", py::module_local(),
                             "The per-token tables of a document mask (doc_mask(cu_doclens, S)): kv_len Long [B], doc_start and doc_end Int [B, S], B, S. "
                             "Built once per batch, passed as doc_mask= to attention and attention_qkv by every layer.")
        .def_readonly("kv_len", &gpu::DocMask::kv_len)
        .def_readonly("doc_start", &gpu::DocMask::doc_start)
        .def_readonly("doc_end", &gpu::DocMask::doc_end)
        .def_readonly("B", &gpu::DocMask::B)
        .def_readonly("S", &gpu::DocMask::S)
        // a mask built with window, prefix_lens or causal: doc_start / doc_end are the keys each query sees (key_lo / key_hi), query_lo / query_hi the
        // queries that see each key; a plain mask has neither, no window and causal False
        .def_property_readonly("key_lo", [](const gpu::DocMask &d) { return d.doc_start; })
        .def_property_readonly("key_hi", [](const gpu::DocMask &d) { return d.doc_end; })
        .def_property_readonly("query_lo", [](const gpu::DocMask &d) -> py::object { return d.span ? py::cast(d.query_lo) : py::none(); })
        .def_property_readonly("query_hi", [](const gpu::DocMask &d) -> py::object { return d.span ? py::cast(d.query_hi) : py::none(); })
        .def_property_readonly("window", [](const gpu::DocMask &d) -> py::object {
            if (d.window_left < 0 && d.window_right < 0) return py::none();
            auto side = [](int64_t w) -> py::object { return w < 0 ? py::object(py::none()) : py::object(py::int_(w)); };
            return py::make_tuple(side(d.window_left), side(d.window_right));
        })
        .def_readonly("causal", &gpu::DocMask::causal)
        .def_readonly("span", &gpu::DocMask::span);
    m.def("doc_mask", [opt, win](const Tensor &cu_doclens, int64_t S, py::object window, py::object prefix_lens, bool causal) {
        if (window.is_none() && prefix_lens.is_none() && !causal) return gpu::doc_mask(cu_doclens, S); // the plain mask: its launch, its tables
        gpu::AttentionWindow w;
        return gpu::doc_mask(cu_doclens, S, win("doc_mask", window, w), opt(prefix_lens), causal);
    }, py::arg("cu_doclens"), py::arg("S"), py::arg("window") = py::none(), py::arg("prefix_lens") = py::none(), py::arg("causal") = false,
          "doc_mask(cu_doclens, S) -> DocMask. cu_doclens: Long [B, n_docs + 1] on the device, the cumulative document lengths of each packed row:\n"
          "cu[b, 0] = 0 and document j of row b holds the tokens cu[b, j] <= m < cu[b, j+1]; a row with fewer documents repeats its last value\n"
          "(a zero-length document owns no token); values are clamped to [0, S], rows must be nondecreasing. Tokens at or beyond cu[b, -1] are\n"
          "in no document. One launch; the DocMask is reused by every layer, forward and backward.\n"
          "doc_mask(cu_doclens, S, window=None, prefix_lens=None, causal=False): with any of the three the mask holds, inside each document, a\n"
          "causal rule (causal=True), a bidirectional prefix per document (prefix_lens: Long [B, n_docs] on the device, clamped to the\n"
          "document; needs causal=True) and a sliding window (window: attention's pair; with causal=True the right side is 0 or None, read as\n"
          "0): query m of document j sees key n of the same document iff (not causal or n <= m or n < start_j + prefix_j) and\n"
          "m - left <= n <= m + right. With prefixes the right side is the causal rule alone, so a token sees the keys of its prefix that its\n"
          "left side reaches. One launch writes four tables: doc_start / doc_end (also key_lo / key_hi), the keys each query sees, and\n"
          "query_lo / query_hi, the queries that see each key; the mask keeps its window and its causal. attention(..., causal=) must repeat\n"
          "the mask's causal. The local layers of a packed batch share one such mask, the global layers a plain one.");
    auto doc = [](const char *op, const py::object &d) -> const gpu::DocMask * {
        if (d.is_none()) return nullptr;
        if (!py::isinstance<gpu::DocMask>(d)) throw py::value_error(std::string(op) + ": doc_mask is a DocMask (doc_mask(cu_doclens, S)) or None");
        return d.cast<const gpu::DocMask *>();
    };
    // softcap = a positive float, sinks = a Float tensor [Hq]: the modifiers of the scores; both None: no modifier, the calls as they were
    auto mod = [opt](const char *op, const py::object &softcap, const py::object &sinks, gpu::AttentionModifiers &out) -> const gpu::AttentionModifiers * {
        if (softcap.is_none() && sinks.is_none()) return nullptr;
        if (!softcap.is_none()) {
            if (!py::isinstance<py::float_>(softcap) && !py::isinstance<py::int_>(softcap))
                throw py::value_error(std::string(op) + ": softcap is a positive float or None");
            out.has_softcap = true;
            out.softcap = softcap.cast<double>();
        }
        out.sinks = opt(sinks);
        return &out;
    };
    m.def("attention", [opt, win, doc, mod](const Tensor &q, const Tensor &k, const Tensor &v, py::object kv_len, bool causal, py::object prefix_len,
                                            py::object window, py::object doc_mask, py::object softcap, py::object sinks) {
        gpu::AttentionWindow w;
        gpu::AttentionModifiers mo;
        return gpu::attention(q, k, v, opt(kv_len), causal, opt(prefix_len), win("attention", window, w), doc("attention", doc_mask),
                              mod("attention", softcap, sinks, mo));
    }, py::arg("q"), py::arg("k"), py::arg("v"), py::arg("kv_len") = py::none(), py::arg("causal") = false, py::arg("prefix_len") = py::none(),
          py::arg("window") = py::none(), py::arg("doc_mask") = py::none(), py::arg("softcap") = py::none(), py::arg("sinks") = py::none(),
          "Softmax attention of q [B, Hq, Sq, D] over k, v [B, Hkv, Skv, D]. kv_len: Long [B], batch b sees keys n < kv_len[b]. causal=True adds\n"
          "the prefix-LM mask: query m sees key n iff n < kv_len[b] and (n < prefix_len[b] or n <= m), top-left aligned; prefix_len: Long [B]\n"
          "or None (no prefix: causal attention over a padded batch), refused with causal=False. A plain causal call without lengths is\n"
          "faster through causal_attention / causal_attention_gqa.\n"
          "window: None, or a pair (left, right) for sliding-window attention: query m sees key n iff n < kv_len[b] and m - left <= n <= m + right,\n"
          "top-left aligned. Each side is a non-negative int or None (unbounded on that side); negative values are refused. causal=True with a\n"
          "window means right = 0 (a right side other than 0 or None is refused); window together with prefix_len is refused. A query that\n"
          "sees no key gives a zero row.\n"
          "doc_mask: None, or a DocMask (doc_mask(cu_doclens, S)) for packed rows: each row holds several documents end to end and query m sees\n"
          "key n iff both lie in the same document (causal=True: and n <= m). Self-attention only (Sq = Skv = S of the mask); doc_mask together\n"
          "with kv_len, prefix_len or window is refused, and so is a mask built for another B, S or device. A token in no document gives a\n"
          "zero row. A window or prefixes INSIDE documents belong to the mask: doc_mask(cu_doclens, S, window=..., prefix_lens=..., causal=...);\n"
          "such a mask holds the causal rule itself, and causal= here must equal the mask's (a mismatch is refused).\n"
          "softcap: None, or a positive finite float: every visible score x = q.k / sqrt(D) becomes softcap * tanh(x / softcap) (logit\n"
          "soft-capping); zero, negative and non-finite values are refused. sinks: None, or a Float tensor [Hq] on q's device (attention\n"
          "sinks): exp(sinks[h]) joins the softmax denominator of every query of head h - a raw logit, neither scaled nor capped - and owns\n"
          "no value row; it is a differentiable input and receives a Float [Hq] gradient. Both compose with every mask above.");
    m.def("attention_qkv", [opt, win, doc, mod](const Tensor &qkv, int64_t B, int64_t S, int64_t H, py::object kv_heads, py::object kv_len, bool causal,
                                                py::object prefix_len, py::object window, py::object doc_mask, py::object softcap, py::object sinks) {
        gpu::AttentionWindow w;
        gpu::AttentionModifiers mo;
        return gpu::attention_qkv(qkv, B, S, H, kv_heads.is_none() ? -1 : kv_heads.cast<int64_t>(), opt(kv_len), causal, opt(prefix_len),
                                  win("attention_qkv", window, w), doc("attention_qkv", doc_mask), mod("attention_qkv", softcap, sinks, mo));
    }, py::arg("qkv"), py::arg("B"), py::arg("S"), py::arg("H"), py::arg("kv_heads") = py::none(), py::arg("kv_len") = py::none(),
          py::arg("causal") = false, py::arg("prefix_len") = py::none(), py::arg("window") = py::none(), py::arg("doc_mask") = py::none(),
          py::arg("softcap") = py::none(), py::arg("sinks") = py::none(),
          "attention on the packed projection [B*S, (H + 2*kv_heads)*D] (columns q | k | v), read in place; the result is [B*S, H*D]. kv_len,\n"
          "causal and prefix_len as in attention (Sq = Skv = S). A plain causal call without lengths is faster through causal_attention_qkv.\n"
          "window: as in attention.\n"
          "doc_mask: as in attention (a DocMask built for this B and S).\n"
          "softcap, sinks: as in attention (sinks is Float [H]).");
    // rotary position embeddings: f64-accurate tables, and the rotation of q and k in place in the packed projection (one launch each way)
    m.def("rope_table", [](int64_t max_positions, int64_t rotary_dim, double base, int device) {
        auto [c, sn] = gpu::rope_table(max_positions, rotary_dim, base, device);
        return py::make_tuple(c, sn);
    }, py::arg("max_positions"), py::arg("rotary_dim"), py::arg("base") = 10000.0, py::arg("device") = 0);
    m.def("rope_qkv", [](const Tensor &qkv, const Tensor &cos, const Tensor &sin, int64_t B, int64_t S, int64_t H, py::object kv_heads, py::object positions,
                         bool interleaved) {
        return gpu::rope_qkv(qkv, cos, sin, B, S, H, kv_heads.is_none() ? -1 : kv_heads.cast<int64_t>(),
                             positions.is_none() ? Tensor() : positions.cast<Tensor>(), interleaved);
    }, py::arg("qkv"), py::arg("cos"), py::arg("sin"), py::arg("B"), py::arg("S"), py::arg("H"), py::arg("kv_heads") = py::none(),
          py::arg("positions") = py::none(), py::arg("interleaved") = false);
    m.def("rope", [](const Tensor &x, const Tensor &cos, const Tensor &sin, py::object positions, bool interleaved) {
        return gpu::rope(x, cos, sin, positions.is_none() ? Tensor() : positions.cast<Tensor>(), interleaved);
    }, py::arg("x"), py::arg("cos"), py::arg("sin"), py::arg("positions") = py::none(), py::arg("interleaved") = false);
    m.def("qk_norm_rope", [](const Tensor &qkv, py::object q_weight, py::object k_weight, py::object cos, py::object sin, int64_t B, int64_t S, int64_t H,
                             py::object kv_heads, py::object positions, bool interleaved, double eps) {
        auto opt = [](const py::object &o) { return o.is_none() ? Tensor() : o.cast<Tensor>(); };
        return gpu::qk_norm_rope(qkv, opt(q_weight), opt(k_weight), opt(cos), opt(sin), B, S, H, kv_heads.is_none() ? -1 : kv_heads.cast<int64_t>(),
                                 opt(positions), interleaved, eps);
    }, py::arg("qkv"), py::arg("q_weight"), py::arg("k_weight"), py::arg("cos"), py::arg("sin"), py::arg("B"), py::arg("S"), py::arg("H"),
          py::arg("kv_heads") = -1, py::arg("positions") = py::none(), py::arg("interleaved") = false, py::arg("eps") = 1e-6,
          "qk_norm_rope(qkv, q_weight, k_weight, cos, sin, B, S, H, kv_heads=-1, positions=None, interleaved=False, eps=1e-6): the per-head "
          "QK-norm of Chameleon / Qwen3 / Gemma-3 / OLMo-2 fused with the rotary embedding, on the contiguous packed projection "
          "[B*S, (H + 2 kv_heads) D] (q | k | v heads; kv_heads = -1 means H). For every q head (q_weight) and every k head (k_weight): "
          "rstd = 1 / sqrt(mean(x^2) + eps), n = x * rstd * w, then the rotation of rope_qkv over the leading rotary_dim dims; v is copied. "
          "Everything is f32 on the stored values with a single rounding, at the store (rms_norm followed by rope_qkv rounds n in between, so "
          "its bits differ). Returns a new packed tensor for attention_qkv, causal_attention_qkv and the GQA operators. cos = sin = None is "
          "the norm alone; a weight may be None (1, no gradient). Differentiable in qkv, q_weight and k_weight (the tables get no gradient): "
          "the backward keeps only its input (qkv, the weights, the tables and the positions) and recomputes rstd. The weight multiplies as "
          "given: for the Gemma convention (1 + w) pass 1 + w.");
    // gated activations (one launch each way; the packed [..., 2F] gate | up projection is read in place): torch's F.gelu argument name
    auto gelu_kind = [](const std::string &approximate) {
        CHECK_FAIL(approximate == "none" || approximate == "tanh", approximate, " is not a valid value for approximate ('none' or 'tanh')");
        return approximate == "tanh" ? KF_ACT_GELU_TANH : KF_ACT_GELU_ERF;
    };
    m.def("swiglu", [](const Tensor &gate, py::object up) { return gpu::glu(KF_ACT_SILU, gate, up.is_none() ? Tensor() : up.cast<Tensor>()); },
          py::arg("gate"), py::arg("up") = py::none());
    m.def("geglu", [gelu_kind](const Tensor &gate, py::object up, const std::string &approximate) {
        return gpu::glu(gelu_kind(approximate), gate, up.is_none() ? Tensor() : up.cast<Tensor>());
    }, py::arg("gate"), py::arg("up") = py::none(), py::arg("approximate") = "none");
    m.def("silu", [](const Tensor &x) { return gpu::activation(KF_ACT_SILU, x); }, py::arg("x"));
    m.def("gelu", [gelu_kind](const Tensor &x, const std::string &approximate) { return gpu::activation(gelu_kind(approximate), x); },
          py::arg("x"), py::arg("approximate") = "none");
    // the expert product of a mixture-of-experts layer: row segments with device-side boundaries, each through its own weight
    m.def("segment_offsets", &gpu::segment_offsets, py::arg("sorted_ids"), py::arg("num_experts"),
          "segment_offsets(sorted_ids, num_experts): Long [num_experts + 1], offsets[e] = the number of the ascending Long ids that are < e, so "
          "expert e owns the sorted rows offsets[e] .. offsets[e + 1]; ids below 0 or at least num_experts fall outside every segment. The "
          "result stays on the device: nothing is read back. In an MoE layer sorted_ids are the keys of the stable sort of the flattened "
          "topk expert ids, and the sort's positions are the permutation that expert_linear's rows follow.");
    m.def("expert_linear", &gpu::expert_linear, py::arg("x"), py::arg("w"), py::arg("offsets"),
          "expert_linear(x [T, Din], w [E, Din, Dout], offsets [E + 1]) -> [T, Dout]: y[r] = x[r] @ w[e] for offsets[e] <= r < offsets[e + 1], "
          "float, half or bfloat16; a row no expert covers is zero and has a zero gradient. Differentiable in x and w (an empty expert's "
          "gradient is zero); offsets (segment_offsets, on the device) gets no gradient. x may be row-pitched, w is contiguous. A layer is "
          "composed from the existing operators: p = softmax(x @ router); gate, ids = p.topk(k); keys, pos = ids.view(-1).sort() (stable); "
          "offsets = segment_offsets(keys, E); xs = embedding(x, pos // k) (the row gather, whose backward is the reproducible index-add); "
          "h = expert_linear(xs, w_gate_up, offsets); a = swiglu(h); ys = expert_linear(a, w_down, offsets); y = sum over k of gate * "
          "embedding(ys, inverse permutation).");
    // the routing around the expert product, on the device: the plan (one sort), the gate, the dispatch and the weighted combine
    py::class_<gpu::MoePlan>(m, "MoePlan", py::module_local(),
                             "The routing of T tokens to k of E experts each (moe_plan(ids, num_experts)): offsets Long [E + 1] (what expert_linear takes; "
                             "offsets[E] = the number of live pairs), row_pair Int [T k] (the pair t k + j in sorted row r), pair_row Int [T, k] (its inverse), "
                             "ids, T, k, E. Built once per layer, used by that layer's forward and backward.")
        .def_readonly("offsets", &gpu::MoePlan::offsets)
        .def_readonly("row_pair", &gpu::MoePlan::row_pair)
        .def_readonly("pair_row", &gpu::MoePlan::pair_row)
        .def_readonly("ids", &gpu::MoePlan::ids)
        .def_readonly("T", &gpu::MoePlan::T)
        .def_readonly("k", &gpu::MoePlan::k)
        .def_readonly("E", &gpu::MoePlan::E);
    auto moe_plan_of = [](const char *op, const py::object &o) -> const gpu::MoePlan & {
        if (!py::isinstance<gpu::MoePlan>(o)) throw py::value_error(std::string(op) + ": plan is a MoePlan (moe_plan(ids, num_experts))");
        return o.cast<const gpu::MoePlan &>();
    };
    m.def("moe_plan", &gpu::moe_plan, py::arg("ids"), py::arg("num_experts"),
          "moe_plan(ids, num_experts) -> MoePlan. ids: Long [T, k] on the device, e.g. p.topk(k, -1, True)[1]. A stable sort of the T k (token, "
          "choice) pairs by expert id, on the device: nothing is read back, so the layer can be captured in a graph. An id outside "
          "[0, num_experts) drops its pair: it sorts behind every expert, expert_linear gives its row zeros and moe_combine skips it. "
          "plan.offsets feeds expert_linear unchanged.");
    m.def("moe_gate", [moe_plan_of](const Tensor &p, const py::object &plan, bool normalize) { return gpu::moe_gate(p, moe_plan_of("moe_gate", plan), normalize); },
          py::arg("p"), py::arg("plan"), py::arg("normalize") = false,
          "moe_gate(p [T, E], plan, normalize=False) -> [T, k]: gate[t, j] = p[t, plan.ids[t, j]] (0 for a dropped pair); normalize=True divides "
          "by their sum over j (f32, in the order j). float, half or bfloat16; p may be row-pitched. Differentiable in p: one launch that "
          "writes all of dp, zero off the chosen columns.");
    m.def("moe_dispatch", [moe_plan_of](const Tensor &x, const py::object &plan) { return gpu::moe_dispatch(x, moe_plan_of("moe_dispatch", plan)); },
          py::arg("x"), py::arg("plan"),
          "moe_dispatch(x [T, d], plan) -> xs [T k, d]: xs[r] = x[plan.row_pair[r] // k], the rows in expert order for expert_linear, bit for "
          "bit. A row-pitched x is read in place. Differentiable in x: dx[t] = the f32 sum over j of dxs[plan.pair_row[t, j]], a gather-sum "
          "(no sort, no atomics, bitwise reproducible).");
    m.def("moe_combine", [moe_plan_of](const Tensor &ys, const py::object &plan, py::object gate) {
        return gpu::moe_combine(ys, moe_plan_of("moe_combine", plan), gate.is_none() ? Tensor() : gate.cast<Tensor>());
    }, py::arg("ys"), py::arg("plan"), py::arg("gate") = py::none(),
          "moe_combine(ys [T k, d], plan, gate=None) -> y [T, d]: y[t] = sum over j of gate[t, j] * ys[plan.pair_row[t, j]], accumulated in "
          "f32 in the order j and rounded once; gate [T, k] (moe_gate) or None (1). Dropped pairs are skipped: neither their row nor their "
          "gate is read. Differentiable in ys and gate in one pass: dys[pair_row[t, j]] = gate[t, j] * dy[t] (zero for a dropped pair), "
          "dgate[t, j] = dy[t] . ys[pair_row[t, j]].");
    // the router in front of the plan, fused: the top-k choice with its gates, and the auxiliary losses
    m.def("moe_route", [](const Tensor &logits, int64_t k, const std::string &score, bool normalize) {
        int s = -1;
        if (score == "softmax") s = KF_MOE_SCORE_SOFTMAX;
        else if (score == "sigmoid") s = KF_MOE_SCORE_SIGMOID;
        CHECK_FAIL(s >= 0, "moe_route: ", score, " is not a valid value for score (softmax, sigmoid)");
        auto out = gpu::moe_route(logits, k, s, normalize);
        return py::make_tuple(out.first, out.second);
    }, py::arg("logits"), py::arg("k"), py::arg("score") = "softmax", py::arg("normalize") = true,
          "moe_route(logits [T, E], k, score='softmax', normalize=True) -> (ids Long [T, k], gate [T, k]) in one launch. ids are the first k "
          "positions of the stable descending order of each row in the sort's key order (-0.0 below +0.0, NaNs by bit pattern, equal values "
          "by lower index): logits.topk(k)[1] bit for bit. gate = softmax(logits)[ids], or sigmoid(logits[ids]) with score='sigmoid', in f32 "
          "with one rounding; normalize=True divides by their sum over j. float, half or bfloat16; E <= 1024, k <= min(E, 64); logits may be "
          "row-pitched. gate is differentiable in logits (one launch that recomputes the row and writes all of dlogits); ids carries no "
          "gradient and feeds moe_plan.");
    m.def("moe_aux_loss", [moe_plan_of](const Tensor &logits, const py::object &plan, double balance_coef, double z_coef, bool return_parts) -> py::object {
        Tensor parts;
        Tensor loss = gpu::moe_aux_loss(logits, moe_plan_of("moe_aux_loss", plan), balance_coef, z_coef, return_parts ? &parts : nullptr);
        if (return_parts) return py::make_tuple(loss, parts);
        return py::cast(loss);
    }, py::arg("logits"), py::arg("plan"), py::arg("balance_coef") = 1e-2, py::arg("z_coef") = 0.0, py::arg("return_parts") = false,
          "moe_aux_loss(logits [T, E], plan, balance_coef=1e-2, z_coef=0.0, return_parts=False) -> Float [1] = balance_coef * L_bal + z_coef * "
          "L_z with p = softmax(logits): L_bal = E / (T k) * sum_e c_e * mean_t p[t, e], c_e = plan.offsets[e + 1] - plan.offsets[e] read on "
          "the device and treated as a constant (the Switch / Megatron normalisation, 1 for uniform routing; HF-Mixtral's value is k times "
          "this); L_z = mean_t logsumexp(logits[t])^2 (ST-MoE). return_parts=True also returns Float [2] = (L_bal, L_z). No atomics: bitwise "
          "reproducible. Differentiable in logits in one pass; the incoming gradient is read from the device.");
    // the distribution over a dimension (an MoE router, sampling, distillation): one launch each way, the backward from the kept result
    m.def("softmax", &gpu::softmax, py::arg("x"), py::arg("dim") = -1, py::arg("scale") = 1.0f,
          "softmax(x, dim=-1, scale=1.0): exp(scale * x) normalised to sum 1 over dimension dim of a float, half or bfloat16 tensor, in f32 "
          "with one rounding per element. scale (1 / temperature) must be finite and > 0. A -inf element gives 0; a row holding a NaN or "
          "+inf, or only -inf, is NaN. The last dimension of a row-strided view is read in place; any other dim is moved last and back. "
          "Differentiable: the backward keeps the result, not x.");
    m.def("log_softmax", &gpu::log_softmax, py::arg("x"), py::arg("dim") = -1, py::arg("scale") = 1.0f,
          "log_softmax(x, dim=-1, scale=1.0): scale * x - log(sum(exp(scale * x))) over dimension dim of a float, half or bfloat16 tensor, in "
          "f32 with one rounding per element and no cancellation at large logits. scale (1 / temperature) must be finite and > 0. A -inf "
          "element stays -inf; a row holding a NaN or +inf, or only -inf, is NaN. Differentiable: the backward keeps the result, not x.");
    // from_numpy for bfloat16: uint16 bit patterns in, a BFloat16 tensor out (the inverse of to_numpy's uint16 view)
    m.def("from_numpy_bf16", [](py::array array, int device) {
        CHECK_FAIL(array.dtype().kind() == 'u' && array.dtype().itemsize() == 2, "from_numpy_bf16 expects uint16 bit patterns");
        py::array c = py::array::ensure(array, py::array::c_style);
        std::vector<int64_t> shape(c.shape(), c.shape() + c.ndim());
        Tensor out = empty(shape, ScalarType::BFloat16, device);
        if (out.numel() > 0) out.copy_from_cpu_ptr(const_cast<void *>(c.data()));
        return out;
    }, py::arg("array"), py::arg("device") = 0);
    m.def("gemm", &gpu::gemm);
    m.def("cat", &gpu::concat);
    m.def("_iter_geometry", &iter_geometry, py::arg("outputs"), py::arg("inputs"), py::arg("is_reduction") = false,
          py::arg("reduce_dim") = 0, py::arg("resize_outputs") = true, py::arg("aliases") = std::vector<int>(), py::arg("check_mem_overlap") = true);
    m.def("_promote_types", &promote_types);
    m.def("_pool_index", &utils::memory::DeviceAllocator::pool_index);
    m.def("release_cached", [](int device) { return utils::memory::DeviceAllocator::GetInstance()->release_cached(device); }, py::arg("device") = 0);
    // test hook (tests/test_gpu_host_api.py: a simulated shortage): refuses to arm unless the process says it is a test
    m.def("_alloc_fail_above", [](size_t bytes) {
        CHECK_FAIL(bytes == 0 || std::getenv("KF_TEST_HOOKS") != nullptr, "_alloc_fail_above is a test hook: set KF_TEST_HOOKS=1");
        utils::memory::DeviceAllocator::GetInstance()->debug_fail_above(bytes);
    });
    m.def("_alloc_oom_retries", []() { return utils::memory::DeviceAllocator::GetInstance()->oom_retries(); });

    py::class_<Tensor>(m, "tensor", py::module_local())
        .def("__copy__", [](const Tensor &self) { return Tensor(self); })
        .def("__deepcopy__", [](const Tensor &self, py::dict) { return Tensor(self); })
        .def("__repr__", &Tensor::to_string)
        .def("defined", &Tensor::defined)
        .def("numpy", [](const Tensor &self) { return to_numpy(self); })
        .def("numel", &Tensor::numel)
        .def("dim", &Tensor::dim)
        .def("device", &Tensor::device)
        .def("shape", [](const Tensor &self, int64_t d) { return self.shape((int)d); })
        .def("sizes", [](const Tensor &self) { return self.sizes(); })
        .def("strides", [](const Tensor &self) { return self.strides(); })
        .def("storage_offset", &Tensor::storage_offset)
        .def("is_contiguous", &Tensor::is_contiguous)
        .def("dtype", &Tensor::dtype)
        .def("item", [](Tensor &self, std::vector<int64_t> indices) -> py::object {
            any_t raw = self.item(indices);
            switch (self.dtype()) {
            case ScalarType::Bool: return py::cast(*reinterpret_cast<uint8_t *>(raw.val) != 0);
            case ScalarType::Byte: return py::cast(*reinterpret_cast<uint8_t *>(raw.val));
            case ScalarType::Char: return py::cast(*reinterpret_cast<int8_t *>(raw.val));
            case ScalarType::Short: return py::cast(*reinterpret_cast<int16_t *>(raw.val));
            case ScalarType::Int: return py::cast(*reinterpret_cast<int32_t *>(raw.val));
            case ScalarType::Long: return py::cast(*reinterpret_cast<int64_t *>(raw.val));
            case ScalarType::Half: return py::cast(dtype::f16_bits_to_float(*reinterpret_cast<uint16_t *>(raw.val)));
            case ScalarType::BFloat16: return py::cast(dtype::bf16_bits_to_float(*reinterpret_cast<uint16_t *>(raw.val)));
            case ScalarType::Float: return py::cast(*reinterpret_cast<float *>(raw.val));
            case ScalarType::Double: return py::cast(*reinterpret_cast<double *>(raw.val));
            default: return py::none();
            }
        })
        .def("fill_", [](Tensor &self, double value) { return self.fill_(any_t{value}); })
        .def("data_ptr", [](Tensor &self) -> uintptr_t { return reinterpret_cast<uintptr_t>(self.data_ptr()); })
        .def("storage_ref_count", &Tensor::storage_ref_count)
        .def("impl_ref_count", &Tensor::impl_ref_count)
        .def("contiguous", &Tensor::contiguous)
        .def("permute", [](Tensor &self, py::args args) {
            CHECK_FAIL((int)args.size() == self.dim());
            return self.permute(args_to_dims(args));
        })
        .def("view", [](Tensor &self, py::args args) { return self.view(args_to_dims(args)); })
        .def("split", &Tensor::split)
        .def("sort", &Tensor::sort)
        .def("topk", &Tensor::topk)
        .def("__getitem__", &get_item)
        .def("__add__", &Tensor::operator+)
        .def("__add__", [](const Tensor &self, double s) { return gpu::add(self, s); })
        .def("__iadd__", &Tensor::operator+=)
        .def("__iadd__", [](Tensor &self, double s) { gpu::add_(self, s); return self; })
        .def("__sub__", &Tensor::operator-)
        .def("__sub__", [](const Tensor &self, double s) { return gpu::sub(self, s); })
        .def("__isub__", &Tensor::operator-=)
        .def("__isub__", [](Tensor &self, double s) { gpu::sub_(self, s); return self; })
        .def("__mul__", &Tensor::operator*)
        .def("__mul__", [](const Tensor &self, double s) { return gpu::mul(self, s); })
        .def("__imul__", &Tensor::operator*=)
        .def("__imul__", [](Tensor &self, double s) { gpu::mul_(self, s); return self; })
        .def("__truediv__", &Tensor::operator/)
        .def("__truediv__", [](const Tensor &self, double s) { return gpu::div(self, s); })
        .def("__itruediv__", &Tensor::operator/=)
        .def("__itruediv__", [](Tensor &self, double s) { gpu::div_(self, s); return self; })
        .def("sum", &Tensor::sum)
        .def("mean", &Tensor::mean)
        .def("mean_var", &Tensor::mean_var)
        .def("norm_stat", &Tensor::norm_stat)
        .def("index_put_", &Tensor::index_put_)
        .def("half", &Tensor::_half)
        .def("bfloat16", &Tensor::_bfloat16)
        .def("float", &Tensor::_float)
        .def("double", &Tensor::_double) // extension: the reference converts to half, bfloat16 and float only
        .def("requires_grad", &Tensor::requires_grad)
        .def("set_requires_grad", &Tensor::set_requires_grad)
        .def("backward", &Tensor::backward)
        // extension: drop the accumulated gradient (an optimizer's zero_grad(set_to_none)); the next backward's first gradient is
        // then taken over without a copy when nothing else refers to it
        .def("zero_grad", [](Tensor &self) { self.impl()->grad_.reset(); })
        .def("grad", [](Tensor &self) {
            if (self.grad() && self.grad()->defined()) return *self.grad();
            return Tensor();
        });
}
