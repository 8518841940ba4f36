// _pcgmix_step: the armed plain splice step of augment() as ONE compiled CPython call.
//
// What augmentations.gate_passes() plus the armed branch of augmentations.splice_plain() do in Python —
// eligibility, probability gate, output tensor, pcgmix_augment_plain_begin_edges, lambda from numpy's
// global stream, partner buffer, pcgmix_augment_plain_finish — is done here.  The tensors are reached through
// libtorch (THPVariable_Unpack and at::Tensor accessors, at::empty_like, c10's current HIP stream): some twenty
// CPython attribute and method calls stood between the call and the launch otherwise, all of them on the
// step's host-GPU loop.  The module therefore links torch's libraries and loads only into a process that has
// imported torch.  numpy objects are reached through their Python methods (they run beside the kernel), and
// the library entry points are called through the addresses the binding takes out of the ctypes.CDLL that
// _lib.load() holds, so both callers use one library instance and one step context.
//
// step() never raises for an input it does not serve: it returns None ("declined") before anything is
// launched and the Python path produces the result or the error it always did.
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <ATen/core/Tensor.h>
#include <ATen/ops/empty_like.h>
#include <c10/hip/HIPStream.h>
#include <torch/csrc/autograd/python_variable.h>

#include <cstdint>
#include <cstdio>
#include <cstring>

#include "pcgmix_hip.h"

namespace {

// ---- what bind() hands over ---------------------------------------------------------------------
decltype(&pcgmix_ctx_gate) fn_gate = nullptr;
decltype(&pcgmix_augment_plain_begin_edges) fn_begin = nullptr;
decltype(&pcgmix_augment_plain_finish) fn_finish = nullptr;
decltype(&pcgmix_augment_plain_abort) fn_abort = nullptr;

PyObject* o_np_random = nullptr;       // the numpy.random module (seed / beta are looked up per call)
PyObject* o_np_empty = nullptr;        // numpy.empty
PyObject* o_np_int64 = nullptr;        // numpy.dtype('int64')
PyObject* o_ndarray_type = nullptr;    // numpy.ndarray
PyObject* o_lib = nullptr;             // the binding module (its TAPE attribute is read per call)
PyObject* o_ctx = nullptr;             // augmentations._CTX: device index -> pcgmix_ctx*
PyObject* o_step_context = nullptr;    // augmentations.step_context
PyObject* o_check_splice = nullptr;    // augmentations._check_splice(err, what)
PyObject* o_check = nullptr;           // _lib.check(err, what)
bool bound = false;

// interned attribute and method names
PyObject *s_seed, *s_beta, *s_TAPE;
PyObject *s_begin_name, *s_finish_name;

struct Ref {                            // owned reference, released at scope exit
  PyObject* p;
  explicit Ref(PyObject* q = nullptr) : p(q) {}
  ~Ref() { Py_XDECREF(p); }
  Ref(const Ref&) = delete;
  Ref& operator=(const Ref&) = delete;
  PyObject* release() { PyObject* q = p; p = nullptr; return q; }
  explicit operator bool() const { return p != nullptr; }
};

PyObject* declined() {                  // whatever made a probe fail is the Python path's to report
  PyErr_Clear();
  Py_RETURN_NONE;
}

// A torch.Tensor of exactly that type (or a Parameter).  A subclass is declined: its methods may be
// overridden (__torch_function__), and torch.empty_like would hand back the subclass.
bool is_tensor(PyObject* o) { return THPVariable_CheckExact(o); }

// The (B, 5) int64 boundaries on the host: a contiguous CPU int64 tensor's storage, or a C-contiguous int64
// ndarray through the buffer protocol (`view` then holds the export until the step is over).
bool frames_address(PyObject* frames, long long B, const int64_t** out, Py_buffer* view, bool* have_view) {
  if (is_tensor(frames)) {
    const at::Tensor& f = THPVariable_Unpack(frames);
    if (!f.defined() || !f.is_cpu() || f.scalar_type() != at::kLong || f.dim() != 2 || f.size(0) != B ||
        f.size(1) != 5 || !f.is_contiguous() || !f.data_ptr())
      return false;
    *out = static_cast<const int64_t*>(f.data_ptr());
    return true;
  }
  if (!PyObject_TypeCheck(frames, reinterpret_cast<PyTypeObject*>(o_ndarray_type))) return false;
  if (PyObject_GetBuffer(frames, view, PyBUF_C_CONTIGUOUS | PyBUF_FORMAT) != 0) return false;
  *have_view = true;
  // numpy spells int64 'l' on LP64 and 'q' where long is 32 bits; byte order marks are absent for native
  const char* f = view->format ? view->format : "";
  const bool i64 = view->itemsize == 8 && ((f[0] == 'l' && sizeof(long) == 8) || f[0] == 'q') && f[1] == '\0';
  if (!i64 || view->ndim != 2 || view->shape[0] != B || view->shape[1] != 5 || !view->buf) return false;
  *out = static_cast<const int64_t*>(view->buf);
  return true;
}

struct BufferHold {                      // releases a Py_buffer export at scope exit
  Py_buffer view;
  bool have = false;
  ~BufferHold() { if (have) PyBuffer_Release(&view); }
};

// the step context of a device: augmentations._CTX.get(index) or step_context(index)
pcgmix_ctx* context_of(PyObject* index) {
  PyObject* v = PyDict_GetItemWithError(o_ctx, index);          // borrowed
  Ref made;
  if (!v) {
    if (PyErr_Occurred()) return nullptr;
    made.p = PyObject_CallOneArg(o_step_context, index);
    if (!made) return nullptr;
    v = made.p;
  }
  return static_cast<pcgmix_ctx*>(PyLong_AsVoidPtr(v));
}

// raise through the binding's own check functions, so that the exception types and messages are theirs
PyObject* raise_status(PyObject* checker, int err, PyObject* what) {
  Ref code(PyLong_FromLong(err));
  if (!code) return nullptr;
  Ref r(PyObject_CallFunctionObjArgs(checker, code.p, what, nullptr));
  if (r) PyErr_Format(PyExc_RuntimeError, "%U failed with status %d", what, err);
  return nullptr;
}

// step(recipe, data, target_ohe, frames, step, host_labels)
//   -> None: declined, nothing launched (the caller takes the Python path)
//   -> (data, target_ohe, [], None): the probability gate rejected the step; data is the object passed in
//   -> (out, target_ohe, mix, None): the armed kernel ran; mix is an int64 ndarray (B,)
PyObject* step(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 6) {
    PyErr_SetString(PyExc_TypeError, "step(recipe, data, target_ohe, frames, step, host_labels)");
    return nullptr;
  }
  if (!bound) {
    PyErr_SetString(PyExc_RuntimeError, "_pcgmix_step.bind() has not been called");
    return nullptr;
  }
  PyObject *recipe = args[0], *data = args[1], *ohe = args[2], *frames = args[3], *step_obj = args[4];

  // 1. eligibility: everything before anything is launched
  if (args[5] != Py_None) return declined();                                  // host_labels
  {
    Ref tape(PyObject_GetAttr(o_lib, s_TAPE));                                // a captured step records its
    if (!tape || tape.p != Py_None) return declined();                       // launches: not from here
  }
  if (!PyTuple_CheckExact(recipe) || PyTuple_GET_SIZE(recipe) != 5) return declined();
  PyObject* alpha_obj = PyTuple_GET_ITEM(recipe, 2);
  const double p = PyFloat_AsDouble(PyTuple_GET_ITEM(recipe, 1));
  const double alpha = PyFloat_AsDouble(alpha_obj);
  const long n_knots = PyLong_AsLong(PyTuple_GET_ITEM(recipe, 4));
  if (PyErr_Occurred() || n_knots != 0 || !(alpha > 0.0)) return declined();
  if (!PyLong_CheckExact(step_obj)) return declined();
  const unsigned long long step_no = PyLong_AsUnsignedLongLong(step_obj);     // negative: OverflowError
  if ((step_no == (unsigned long long)-1 && PyErr_Occurred()) || step_no > 0xFFFFFFFFull) return declined();

  if (!is_tensor(data) || !is_tensor(ohe)) return declined();
  long long B = 0, C = 0, T = 0, K = 0;
  BufferHold hold;
  const int64_t* fr = nullptr;
  void *x = nullptr, *lab = nullptr;
  int device_index = -1;
  try {                                   // whatever torch throws here is the Python path's to report
    const at::Tensor& d = THPVariable_Unpack(data);
    const at::Tensor& o = THPVariable_Unpack(ohe);
    if (!d.defined() || !d.is_cuda() || d.scalar_type() != at::kFloat || d.dim() != 3 || d.size(0) <= 0 ||
        !d.is_contiguous())
      return declined();
    if (!o.defined() || !o.is_cuda() || o.scalar_type() != at::kLong || o.dim() != 2 || o.size(0) != d.size(0) ||
        !o.is_contiguous())
      return declined();
    B = d.size(0), C = d.size(1), T = d.size(2), K = o.size(1);
    if (B > INT32_MAX || C > INT32_MAX || T > INT32_MAX || K > INT32_MAX) return declined();
    if (!frames_address(frames, B, &fr, &hold.view, &hold.have)) return declined();
    x = d.data_ptr();
    lab = o.data_ptr();
    device_index = d.device().index();
  } catch (...) {
    return declined();
  }
  if (device_index < 0) return declined();
  Ref index(PyLong_FromLong(device_index));
  if (!index) return declined();
  pcgmix_ctx* ctx = context_of(index.p);
  if (!ctx) return PyErr_Occurred() ? nullptr : declined();

  // 2. the probability gate: random.Random(step).uniform(0, 1) < p, in the step context
  if (p < 1.0 && !(fn_gate(ctx, step_no) < p)) {
    Ref none_mix(PyList_New(0));
    if (!none_mix) return nullptr;
    return PyTuple_Pack(4, data, ohe, none_mix.p, Py_None);
  }

  // 3. the output, the stream, the launch
  Ref out;
  void* y = nullptr;
  pcgmix_stream_t stream = nullptr;
  try {
    at::Tensor made = at::empty_like(THPVariable_Unpack(data));
    y = made.data_ptr();
    stream = static_cast<pcgmix_stream_t>(
        c10::hip::getCurrentHIPStream(static_cast<c10::DeviceIndex>(device_index)).stream());
    out.p = THPVariable_Wrap(std::move(made));         // wrapped once, for the return tuple
  } catch (...) {
    return declined();                                  // nothing launched: torch.empty_like reports it
  }
  if (!out) return nullptr;
  int err;
  Py_BEGIN_ALLOW_THREADS
  err = fn_begin(ctx, static_cast<const float*>(x), static_cast<float*>(y), static_cast<const int64_t*>(lab),
                 (int)K, (int)B, (int)C, (int)T, fr, stream);
  Py_END_ALLOW_THREADS
  if (err == PCGMIX_NOT_ARMED) return declined();         // nothing was enqueued: the one-call route, in Python
  if (err) return raise_status(o_check, err, s_begin_name);

  // 4.-6. a kernel is waiting from here on: every way out without finish releases it
  Ref mix;
  Py_buffer mv;
  bool have_mv = false;
  float lam = 0.f;
  bool ok = false;
  do {
    Ref seed(PyObject_GetAttr(o_np_random, s_seed));       // looked up per call: a patched attribute counts
    if (!seed) break;
    Ref seeded(PyObject_CallOneArg(seed.p, step_obj));
    if (!seeded) break;
    Ref beta(PyObject_GetAttr(o_np_random, s_beta));
    if (!beta) break;
    Ref drawn(PyObject_CallFunctionObjArgs(beta.p, alpha_obj, alpha_obj, nullptr));
    if (!drawn) break;
    const double lam64 = PyFloat_AsDouble(drawn.p);
    if (lam64 == -1.0 && PyErr_Occurred()) break;
    lam = (float)lam64;                                     // rounds like ctypes.c_float / np.float32
    Ref rows(PyLong_FromLongLong(B));
    if (!rows) break;
    mix.p = PyObject_CallFunctionObjArgs(o_np_empty, rows.p, o_np_int64, nullptr);
    if (!mix) break;
    if (PyObject_GetBuffer(mix.p, &mv, PyBUF_WRITABLE) != 0) break;
    have_mv = true;
    if (mv.len != (Py_ssize_t)(B * 8) || !mv.buf) {
      PyErr_SetString(PyExc_RuntimeError, "numpy.empty did not return B int64");
      break;
    }
    ok = true;
  } while (false);
  if (!ok) {
    if (have_mv) PyBuffer_Release(&mv);
    PyObject *et, *ev, *tb;
    PyErr_Fetch(&et, &ev, &tb);
    Py_BEGIN_ALLOW_THREADS
    (void)fn_abort(ctx);
    Py_END_ALLOW_THREADS
    PyErr_Restore(et, ev, tb);
    return nullptr;
  }
  Py_BEGIN_ALLOW_THREADS                                    // the label wait may take milliseconds
  err = fn_finish(ctx, fr, step_no, lam, static_cast<int64_t*>(mv.buf));
  Py_END_ALLOW_THREADS
  PyBuffer_Release(&mv);
  if (err) return raise_status(o_check_splice, err, s_finish_name);   // (finish has released the kernel)

  // 7. the reference's return tuple
  return PyTuple_Pack(4, out.p, ohe, mix.p, Py_None);
}

bool take(PyObject* d, const char* key, PyObject** slot) {
  PyObject* v = PyDict_GetItemString(d, key);               // borrowed
  if (!v) {
    PyErr_Format(PyExc_KeyError, "_pcgmix_step.bind: missing %s", key);
    return false;
  }
  Py_INCREF(v);
  Py_XSETREF(*slot, v);
  return true;
}

template <class F>
bool take_address(PyObject* d, const char* key, F* slot) {
  PyObject* v = PyDict_GetItemString(d, key);
  if (!v) {
    PyErr_Format(PyExc_KeyError, "_pcgmix_step.bind: missing the address of %s", key);
    return false;
  }
  void* p = PyLong_AsVoidPtr(v);
  if (!p) {
    if (!PyErr_Occurred()) PyErr_Format(PyExc_ValueError, "_pcgmix_step.bind: %s is a null address", key);
    return false;
  }
  std::memcpy(slot, &p, sizeof(p));
  return true;
}

// bind(objects: dict): the library entry points as integer addresses (from the loaded ctypes.CDLL) and the
// Python objects step() works with; see augmentations._bind_native_step for the keys.
PyObject* bind(PyObject*, PyObject* d) {
  if (!PyDict_Check(d)) {
    PyErr_SetString(PyExc_TypeError, "bind() takes one dict");
    return nullptr;
  }
  bound = false;
  if (!take_address(d, "pcgmix_ctx_gate", &fn_gate) ||
      !take_address(d, "pcgmix_augment_plain_begin_edges", &fn_begin) ||
      !take_address(d, "pcgmix_augment_plain_finish", &fn_finish) ||
      !take_address(d, "pcgmix_augment_plain_abort", &fn_abort) ||
      !take(d, "np_random", &o_np_random) || !take(d, "np_empty", &o_np_empty) ||
      !take(d, "np_int64", &o_np_int64) || !take(d, "ndarray", &o_ndarray_type) || !take(d, "lib", &o_lib) ||
      !take(d, "contexts", &o_ctx) || !take(d, "step_context", &o_step_context) ||
      !take(d, "check_splice", &o_check_splice) || !take(d, "check", &o_check))
    return nullptr;
  if (!PyType_Check(o_ndarray_type) || !PyDict_Check(o_ctx)) {
    PyErr_SetString(PyExc_TypeError, "_pcgmix_step.bind: ndarray must be a type, contexts a dict");
    return nullptr;
  }
  bound = true;
  Py_RETURN_NONE;
}

PyMethodDef methods[] = {
    {"step", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(step)), METH_FASTCALL,
     "step(recipe, data, target_ohe, frames, step, host_labels) -> None (declined) | the augment() 4-tuple"},
    {"bind", bind, METH_O, "bind(objects): hand over the library entry points and the Python callables"},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef moduledef = {PyModuleDef_HEAD_INIT, "_pcgmix_step",
                         "The armed plain splice step of augment() from one compiled entry point.", -1, methods,
                         nullptr, nullptr, nullptr, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__pcgmix_step(void) {
  // the file name carries no ABI tag: refuse an interpreter of another minor version than the headers'
  int major = 0, minor = 0;
  if (std::sscanf(Py_GetVersion(), "%d.%d", &major, &minor) != 2 || major != PY_MAJOR_VERSION ||
      minor != PY_MINOR_VERSION) {
    PyErr_Format(PyExc_ImportError, "_pcgmix_step was built for Python %d.%d, this is %s: rebuild it (make)",
                 PY_MAJOR_VERSION, PY_MINOR_VERSION, Py_GetVersion());
    return nullptr;
  }
  // torch's Python layer must be up: THPVariable_CheckExact compares against the classes `import torch` registers
  {
    Ref name(PyUnicode_FromString("torch"));
    Ref torch_module(name ? PyImport_GetModule(name.p) : nullptr);
    if (!torch_module) {
      if (!PyErr_Occurred()) PyErr_SetString(PyExc_ImportError, "_pcgmix_step needs torch imported first");
      return nullptr;
    }
  }
  struct { PyObject** slot; const char* text; } names[] = {
      {&s_seed, "seed"}, {&s_beta, "beta"}, {&s_TAPE, "TAPE"}, {&s_begin_name, "pcgmix_augment_plain_begin_edges"},
      {&s_finish_name, "pcgmix_augment_plain_finish"}};
  for (auto& n : names)
    if (!(*n.slot = PyUnicode_InternFromString(n.text))) return nullptr;
  PyObject* m = PyModule_Create(&moduledef);
  if (m && PyModule_AddIntConstant(m, "ABI_VERSION", PCGMIX_ABI_VERSION) != 0) {
    Py_DECREF(m);
    return nullptr;
  }
  return m;
}
