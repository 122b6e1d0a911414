"""YOLO-mode model for ObjectDetector (mode="yolo"): YOLOv8n topology on the library's MFMA conv path.

The reference calls ultralytics `YOLO("yolov8n.pt")(frame)` (detector.py:77-84,103-123); neither the
package nor the weight file can be shipped, so this model takes its parameters from
  * a YOLOv8n `state_dict` file with ultralytics' key names (`model.0.conv.weight`, `model.0.bn.running_mean`, ...,
    `model.22.cv3.2.2.bias`): `.pt` / `.pth` / `.bin` read with `torch.load(weights_only=True)`, `.safetensors`, or an
    `.npz` of such arrays -- `torch.save(YOLO("yolov8n.pt").model.state_dict(), "yolov8n_sd.pt")` on a machine with
    ultralytics produces one (the pickled `DetectionModel` inside `yolov8n.pt` itself needs that package to load),
  * a `.npy` / `.npz` file holding the flat float32 vector in the order of `conv_specs()`, or
  * the pseudo path "random" / "random:<seed>" -> seeded He-normal weights with non-trivial BatchNorm
    statistics (BASELINE config 3: "random-init nano backbone").
Any other path that does not exist raises FileNotFoundError, which ObjectDetector turns into the
reference's graceful fallback to simulated mode.

Parameter order: for every convolution of conv_specs(), weight[cout][cin][k][k] followed by BatchNorm
(gamma, beta, running_mean, running_var) -- or by the bias for the two plain Conv2d that end each head branch.
"""
import ctypes as C
import os

import numpy as np
import torch

from .. import _native as nat
from .._dev import Dev

NC, REG_MAX = 80, 16
CONF_THRES, IOU_THRES, MAX_DET = 0.25, 0.7, 300          # ultralytics predict defaults

COCO_NAMES = ("person bicycle car motorcycle airplane bus train truck boat traffic_light fire_hydrant stop_sign "
              "parking_meter bench bird cat dog horse sheep cow elephant bear zebra giraffe backpack umbrella handbag "
              "tie suitcase frisbee skis snowboard sports_ball kite baseball_bat baseball_glove skateboard surfboard "
              "tennis_racket bottle wine_glass cup fork knife spoon bowl banana apple sandwich orange broccoli carrot "
              "hot_dog pizza donut cake chair couch potted_plant bed dining_table toilet tv laptop mouse remote "
              "keyboard cell_phone microwave oven toaster sink refrigerator book clock vase scissors teddy_bear "
              "hair_drier toothbrush").split()


def _c2f(c1, c2, n):
    c = c2 // 2
    return [(c1, 2 * c, 1, 1, True)] + [(c, c, 3, 1, True)] * (2 * n) + [((2 + n) * c, c2, 1, 1, True)]


def conv_specs():
    """[(cin, cout, k, stride, has_bn_act)] in execution order (yolov8.yaml, scale n)."""
    s = [(3, 16, 3, 2, True), (16, 32, 3, 2, True)] + _c2f(32, 32, 1)
    s += [(32, 64, 3, 2, True)] + _c2f(64, 64, 2) + [(64, 128, 3, 2, True)] + _c2f(128, 128, 2)
    s += [(128, 256, 3, 2, True)] + _c2f(256, 256, 1) + [(256, 128, 1, 1, True), (512, 256, 1, 1, True)]
    s += _c2f(384, 128, 1) + _c2f(192, 64, 1) + [(64, 64, 3, 2, True)] + _c2f(192, 128, 1)
    s += [(128, 128, 3, 2, True)] + _c2f(384, 256, 1)
    for ch in (64, 128, 256):
        s += [(ch, 64, 3, 1, True), (64, 64, 3, 1, True), (64, 4 * REG_MAX, 1, 1, False)]
        s += [(ch, NC, 3, 1, True), (NC, NC, 3, 1, True), (NC, NC, 1, 1, False)]
    return s


def random_params(seed=0):
    rs = np.random.RandomState(seed)
    parts = []
    for cin, cout, k, _, bn in conv_specs():
        parts.append((rs.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / (cin * k * k))).astype(np.float32).ravel())
        if bn:
            parts += [rs.uniform(0.8, 1.2, cout).astype(np.float32), rs.uniform(-0.1, 0.1, cout).astype(np.float32),
                      rs.uniform(-0.1, 0.1, cout).astype(np.float32), rs.uniform(0.8, 1.2, cout).astype(np.float32)]
        else:
            parts.append(rs.uniform(-1.0, 1.0, cout).astype(np.float32))
    return np.concatenate(parts)


def ultralytics_layer_names():
    """The module path of every convolution of conv_specs(), in that order, in ultralytics' YOLOv8n `state_dict`
    (`model.<layer>.…`; a Conv block holds `.conv.weight` + `.bn.{weight,bias,running_mean,running_var}`, the two plain
    Conv2d that end a Detect branch hold `.weight` + `.bias`) -- yolov8.yaml layer numbers, nn/modules/{conv,block,head}.py:
    C2f = cv1, m.<i>.cv1, m.<i>.cv2, cv2; SPPF = cv1, cv2; Detect = cv2.<level>.<0..2> (box), cv3.<level>.<0..2> (class)."""
    def c2f(layer, n):
        return (["%d.cv1" % layer] + [q for i in range(n) for q in ("%d.m.%d.cv1" % (layer, i), "%d.m.%d.cv2" % (layer, i))]
                + ["%d.cv2" % layer])
    names = ["0", "1"] + c2f(2, 1) + ["3"] + c2f(4, 2) + ["5"] + c2f(6, 2) + ["7"] + c2f(8, 1) + ["9.cv1", "9.cv2"]
    names += c2f(12, 1) + c2f(15, 1) + ["16"] + c2f(18, 1) + ["19"] + c2f(21, 1)
    for lvl in range(3):
        names += ["22.cv2.%d.%d" % (lvl, j) for j in range(3)] + ["22.cv3.%d.%d" % (lvl, j) for j in range(3)]
    return names


def params_from_state_dict(sd):
    """Flat parameter vector (the order of conv_specs()) from a YOLOv8n `state_dict` with ultralytics' key names
    (detector.py:77-84 loads such a model through `YOLO(model_path)`).  Keys may carry any number of leading `model.` /
    `module.` prefixes; `num_batches_tracked` and the constant DFL convolution (`22.dfl.conv.weight`, arange(16)) are
    ignored; every shape is checked.  BatchNorm is folded later by the library (eps 1e-3, ultralytics' Conv default)."""
    import re
    flat = {}
    for k, v in sd.items():
        k = re.sub(r"^(?:(?:model|module)\.)+", "", k)
        flat[k] = v
    specs, names = conv_specs(), ultralytics_layer_names()
    assert len(specs) == len(names)

    def get(key, shape):
        if key not in flat:
            raise KeyError("state_dict has no %r (a YOLOv8n checkpoint's state_dict is expected)" % ("model." + key))
        a = flat[key]
        a = a.detach().cpu().float().numpy() if hasattr(a, "detach") else np.asarray(a, np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError("%s has shape %s, YOLOv8n (scale n) needs %s" % (key, tuple(a.shape), tuple(shape)))
        return np.ascontiguousarray(a, np.float32).ravel()
    parts = []
    for (cin, cout, k, _, bn), name in zip(specs, names):
        if bn:
            parts.append(get(name + ".conv.weight", (cout, cin, k, k)))
            parts += [get(name + ".bn." + q, (cout,)) for q in ("weight", "bias", "running_mean", "running_var")]
        else:
            parts += [get(name + ".weight", (cout, cin, k, k)), get(name + ".bias", (cout,))]
    return np.concatenate(parts)


def state_dict_from_params(params, prefix="model."):
    """Inverse of params_from_state_dict (NumPy arrays under ultralytics' key names): lets a parameter vector of this
    project be handed to code that expects a YOLOv8n state_dict, and is what the round-trip test uses."""
    params = np.asarray(params, np.float32).ravel()
    sd, pos = {}, 0
    for (cin, cout, k, _, bn), name in zip(conv_specs(), ultralytics_layer_names()):
        nw = cout * cin * k * k
        w = params[pos:pos + nw].reshape(cout, cin, k, k)
        pos += nw
        if bn:
            sd[prefix + name + ".conv.weight"] = w
            for q in ("weight", "bias", "running_mean", "running_var"):
                sd[prefix + name + ".bn." + q] = params[pos:pos + cout]
                pos += cout
        else:
            sd[prefix + name + ".weight"] = w
            sd[prefix + name + ".bias"] = params[pos:pos + cout]
            pos += cout
    assert pos == params.size
    return sd


def _load_checkpoint(model_path):
    """A torch file (`.pt` / `.pth` / `.bin`) or `.safetensors` -> state_dict.  Only plain tensor containers are read
    (`weights_only=True`): a state_dict, or a dict holding one under "state_dict" / "model_state_dict" / "model".  An
    ultralytics training checkpoint pickles the whole `DetectionModel` object, which cannot be rebuilt without that package --
    save `YOLO("yolov8n.pt").model.state_dict()` once instead."""
    if model_path.endswith(".safetensors"):
        from safetensors.numpy import load_file
        return load_file(model_path)
    try:
        obj = torch.load(model_path, map_location="cpu", weights_only=True)
    except Exception as e:                                  # pickled module classes (ultralytics.nn.tasks.DetectionModel, ...)
        raise FileNotFoundError("%r is not a plain state_dict file (%s: %s); export one with "
                                "torch.save(YOLO(path).model.state_dict(), out)" % (model_path, type(e).__name__, str(e)[:120]))
    for key in ("state_dict", "model_state_dict", "model"):
        if isinstance(obj, dict) and isinstance(obj.get(key), dict):
            obj = obj[key]
    if not isinstance(obj, dict):
        raise FileNotFoundError("%r holds a %s, not a state_dict" % (model_path, type(obj).__name__))
    return obj


def load_params(model_path):
    if model_path.startswith("random"):
        seed = int(model_path.split(":")[1]) if ":" in model_path else 0
        return random_params(seed)
    if not os.path.exists(model_path):
        raise FileNotFoundError("model file %r not found (pass a YOLOv8n state_dict file (.pt/.pth/.safetensors), a "
                                ".npy/.npz parameter vector or 'random[:seed]')" % model_path)
    if model_path.endswith(".npz"):
        z = np.load(model_path)
        if len(z.files) > 1:                                # a state_dict saved with np.savez
            return params_from_state_dict({k: z[k] for k in z.files})
        return np.ascontiguousarray(z[z.files[0]], np.float32).ravel()
    if model_path.endswith(".npy"):
        return np.ascontiguousarray(np.load(model_path), np.float32).ravel()
    return params_from_state_dict(_load_checkpoint(model_path))


class _OwnStream:
    """A Dev with a stream of its own (stream capture needs a non-default stream; the per-frame detector call keeps its upload,
    its graph replay and its wait on it)."""

    def __init__(self, dev):
        self.index, self.device, self.ctx, self.lib = dev.index, dev.device, dev.ctx, dev.lib
        self._stream = torch.cuda.Stream(device=dev.device)

    @property
    def stream(self):
        return nat.stream_handle(self._stream)

    def sync(self):
        self._stream.synchronize()


class YoloV8n:
    def __init__(self, model_path="random", device=0, batch=1, keep_logits=False, precision="fp16"):
        """keep_logits: test hook -- the head also writes its float32 logits (tensor ids 100-105) and the stand-alone decode
        runs on them (ids 120-122); normally the decode happens in the head's last convolutions and no logits exist.
        precision: "fp16" -- IEEE-half tensors / weights / MFMA operands with float32 accumulation, the fused production path;
        "fp32" -- the reference's own arithmetic (ultralytics on torch float32, detector.py:103-123): float32 everywhere on
        v_mfma_f32_16x16x4_f32, one generic kernel per layer, logits always kept (ids 100-105)."""
        if precision not in ("fp16", "fp32"):
            raise ValueError("precision must be 'fp16' or 'fp32', got %r" % (precision,))
        self._dev = Dev(device)
        self.keep_logits = keep_logits
        self.params = load_params(model_path)
        n = int(self._dev.lib.av_yolo_param_count())
        if self.params.size != n:
            raise ValueError("parameter vector has %d floats, the YOLOv8n graph needs %d" % (self.params.size, n))
        self.names = dict(enumerate(COCO_NAMES))
        self.batch = batch
        self.precision = precision
        self._h = None
        self._shape = None
        self._io_in = self._io_out = None      # per-frame call: pinned upload buffer, host-mapped result buffer
        self._io_shape = None
        # per-frame call (batch 1): the whole forward -- ~56 launches on two lanes -- is captured into ONE hipGraph after the first
        # eager call and replayed from then on (demo.py:107 calls the detector once per frame: launch overhead, not kernel time,
        # is what a single 384x640 image costs).  AVHOT_YOLO_NO_GRAPH=1 keeps the eager launches.
        self._gdev = None
        self._graphs = {}                      # (conf, iou) -> graph id, for the current shape
        self._warm = set()
        self.use_graph = os.environ.get("AVHOT_YOLO_NO_GRAPH", "0") != "1"

    def _prepare(self, h, w):
        if self._shape == (h, w):
            return
        d = self._dev
        self.close()
        hd = C.c_void_p()
        nat.check(d.lib.av_yolo_create_ex(d.ctx.handle, self.batch, h, w, self.params.ctypes.data_as(C.c_void_p),
                                          self.params.size, 1 if self.precision == "fp32" else 0, C.byref(hd)))
        self._h = hd
        self._shape = (h, w)
        if self.keep_logits:
            nat.check(d.lib.av_yolo_keep_logits(hd, 1))
        B = self.batch
        self._frames = d.empty((B, h, w, 3), torch.uint8)
        self._n = d.zeros(B, torch.int32)
        self._box = d.zeros((B, MAX_DET, 4), torch.float32)
        self._conf = d.zeros((B, MAX_DET), torch.float32)
        self._cls = d.zeros((B, MAX_DET), torch.int32)

    def dims(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        nat.check(self._dev.lib.av_yolo_dims(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def forward_device(self, frames_dev, conf=CONF_THRES, iou=IOU_THRES):
        """frames_dev: uint8 [batch, h, w, 3] device tensor.  Enqueues the whole detector; results stay on device."""
        d = self._dev
        nat.check(d.lib.av_yolo_forward(self._h, d.stream, nat.ptr(frames_dev), conf, iou, MAX_DET, nat.ptr(self._n),
                                        nat.ptr(self._box), nat.ptr(self._conf), nat.ptr(self._cls)))

    def detect(self, frame, conf=CONF_THRES, iou=IOU_THRES):
        """One BGR frame -> (boxes float32[n,4] xyxy in frame pixels, conf[n], cls[n]).  The per-frame call of the drop-in
        class: the frame goes up through one pinned buffer (host copy and DMA pipelined in pieces), the detections come back
        through one host-mapped buffer the NMS kernel writes directly (no copy commands, no .item(): one polling wait)."""
        frame = np.ascontiguousarray(frame, np.uint8)
        h, w = frame.shape[:2]
        self._prepare(h, w)
        if self.batch != 1:
            self._frames[0].copy_(torch.as_tensor(frame))
            self.forward_device(self._frames, conf, iou)
            n = int(self._n[0].item())
            return (self._box[0, :n].cpu().numpy(), self._conf[0, :n].cpu().numpy(), self._cls[0, :n].cpu().numpy())
        if self._gdev is None:
            self._gdev = _OwnStream(self._dev)
        d = self._gdev
        if self._io_shape != (h, w):
            from .._dev import Packed
            for io in (self._io_in, self._io_out):
                if io is not None:
                    io.close()
            self._io_in = Packed(d, [("frame", np.uint8, (h, w, 3))], mapped=False)
            self._io_out = Packed(d, [("n", np.int32, (1,)), ("box", np.float32, (MAX_DET, 4)), ("conf", np.float32, (MAX_DET,)),
                                      ("cls", np.int32, (MAX_DET,))], mapped=True)
            self._io_shape = (h, w)
        self._io_in.upload_from("frame", frame)
        o = self._io_out

        def enqueue():
            nat.check(d.lib.av_yolo_forward(self._h, d.stream, self._io_in.ptr("frame"), conf, iou, MAX_DET, o.ptr("n"), o.ptr("box"),
                                            o.ptr("conf"), o.ptr("cls")))
        key = (float(conf), float(iou))
        gid = self._graphs.get(key)
        if gid is None and self.use_graph and key in self._warm and not self.keep_logits and self.precision == "fp16":
            # second call with these thresholds: every one-time host action of the forward (symbol uploads, attributes) is behind us
            g = C.c_int(-1)
            nat.check(d.lib.av_graph_begin(d.ctx.handle, d.stream))
            try:
                enqueue()
            finally:
                nat.check(d.lib.av_graph_end(d.ctx.handle, d.stream, C.byref(g)))
            gid = self._graphs[key] = g.value
        if gid is not None:
            nat.check(d.lib.av_graph_launch(d.ctx.handle, gid, d.stream))
        else:
            enqueue()
            self._warm.add(key)
        o.download()
        n = int(o.h["n"][0])
        return o.h["box"][:n].copy(), o.h["conf"][:n].copy(), o.h["cls"][:n].copy()

    def tensor(self, tid, image=0):
        """Host copy (float32, [H, W, C]) of an intermediate tensor of one image of the batch, or of all images
        ([batch, H, W, C]) with image=None (test hook)."""
        p, H, W, Cc, cs, co = C.c_void_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        nat.check(self._dev.lib.av_yolo_tensor(self._h, tid, C.byref(p), C.byref(H), C.byref(W), C.byref(Cc), C.byref(cs),
                                               C.byref(co)))
        if 100 <= tid < 106 and not (self.keep_logits or self.precision == "fp32"):
            raise RuntimeError("head logits exist only in a YoloV8n(keep_logits=True) or in float32 mode")
        n = self.batch * H.value * W.value * cs.value
        t = torch.empty(n, dtype=torch.float32 if (tid >= 100 or self.precision == "fp32") else torch.int16, device=self._dev.device)
        nbytes = t.numel() * t.element_size()
        self._dev.sync()
        rc = _memcpy_d2d(t.data_ptr(), p.value, nbytes)      # the tensor lives in library-owned memory
        if rc != 0:
            raise RuntimeError("hipMemcpy failed (%d)" % rc)
        arr = t.cpu().numpy().reshape(self.batch, H.value, W.value, cs.value)[..., co.value:co.value + Cc.value]
        if image is not None:
            arr = arr[image]
        if tid in (112, 122):
            return np.ascontiguousarray(arr).view(np.int32)
        if tid >= 100 or self.precision == "fp32":
            return arr.astype(np.float32)
        if self.precision == "bf16":                       # (a library built with bf16 activations: comparison runs only)
            return (arr.astype(np.uint16).astype(np.uint32) << 16).view(np.float32)
        return np.ascontiguousarray(arr).view(np.float16).astype(np.float32)

    def ops(self):
        """The ops of the network as the library built them, one per layer in execution order (test hook av_yolo_op): a list of
        nat.YoloOpInfo.  Reads nothing from the device."""
        n = C.c_int()
        nat.check(self._dev.lib.av_yolo_op_count(self._h, C.byref(n)))
        out = []
        for k in range(n.value):
            info = nat.YoloOpInfo()
            nat.check(self._dev.lib.av_yolo_op(self._h, k, C.byref(info)))
            out.append(info)
        return out

    def _read(self, ptr, count, dtype):
        """Host copy of `count` elements of library-owned device memory."""
        t = torch.empty(count, dtype=dtype, device=self._dev.device)
        self._dev.sync()
        rc = _memcpy_d2d(t.data_ptr(), ptr, t.numel() * t.element_size())
        if rc != 0:
            raise RuntimeError("hipMemcpy failed (%d)" % rc)
        return t.cpu().numpy()

    def read_slice(self, s):
        """Host copy of a nat.YoloSlice of an op, all images: float32 or float16 [batch, H, W, c] (test hook)."""
        a = self._read(s.ptr, self.batch * s.H * s.W * s.cstride, torch.float32 if s.f32 else torch.float16)
        return np.ascontiguousarray(a.reshape(self.batch, s.H, s.W, s.cstride)[..., s.coff:s.coff + s.c])

    def read_weights(self, op):
        """Host copy of a convolution op's folded weights, float32 or float16 [cout, kpad], and of its float32 bias [cout] (test hook)."""
        w = self._read(op.wgt, op.cout * op.kpad, torch.float32 if op.wgt_f32 else torch.float16).reshape(op.cout, op.kpad)
        return w, self._read(op.bias, op.cout, torch.float32)

    def close(self):
        if self._h is not None:
            self._dev.sync()
            if self._gdev is not None:
                self._gdev.sync()
            for gid in self._graphs.values():           # the graphs hold this handle's buffers and kernel arguments
                self._dev.lib.av_graph_destroy(self._dev.ctx.handle, gid)
            self._graphs, self._warm = {}, set()
            self._dev.lib.av_yolo_destroy(self._h)
            self._h = None
        for io in (getattr(self, "_io_in", None), getattr(self, "_io_out", None)):
            if io is not None:
                io.close()
        self._io_in = self._io_out = None
        self._io_shape = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _memcpy_d2d(dst, src, nbytes):
    import ctypes
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip.hipMemcpy(dst, src, nbytes, 3)      # hipMemcpyDeviceToDevice
