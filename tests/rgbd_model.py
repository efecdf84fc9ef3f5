"""numpy restatement of Tracking::GrabImageRGBD (S/Tracking.cc:1086-1142) and of the RGB-D Frame constructor (S/Frame.cc:174-257,
ComputeStereoFromRGBD :966-988), built from what the oracle already has (extraction, undistortion, image bounds, grid) plus the three
pieces that are new: the colour -> gray formula, imDepth.convertTo and the depth lookup, written out in integer / float32 numpy.

Pinned arithmetic (OpenCV is not part of this project):
  * 8-bit colour -> gray is OpenCV's fixed-point form (R * 4899 + G * 9617 + B * 1868 + 8192) >> 14; the channel order comes from mbRGB,
    a fourth channel is ignored.
  * convertTo(CV_32F, factor) is ONE float32 product per pixel, (float)raw * factor, for 16-bit unsigned and for float input; it runs
    when fabs(factor - 1.0f) > 1e-5 or the image is not CV_32F.  Converting only the values that are read gives the same bits.
  * imDepth.at<float>(v, u) takes int arguments: the float keypoint coordinates truncate.
"""
import numpy as np

from multi_orbslam3_amd import views
from oracle import binding as ob

F32 = np.float32


def depth_map_factor(yaml_value):
    """mDepthMapFactor as Tracking holds it (S/Tracking.cc:166-172)."""
    f = F32(yaml_value)
    if abs(f) < 1e-5:
        return F32(1.0)
    return F32(F32(1.0) / f)


def gray_from_color(img, rgb_order):
    """cvtColor(RGB2GRAY / BGR2GRAY / RGBA2GRAY / BGRA2GRAY) on H x W x 3|4 uint8."""
    a = img.astype(np.int64)
    c0, g, c2 = a[..., 0], a[..., 1], a[..., 2]
    r, b = (c0, c2) if rgb_order else (c2, c0)
    return ((r * 4899 + g * 9617 + b * 1868 + 8192) >> 14).astype(np.uint8)


def needs_convert(depth_dtype, factor):
    """The condition of S/Tracking.cc:1107."""
    return bool(abs(F32(F32(factor) - F32(1.0))) > 1e-5) or np.dtype(depth_dtype) != np.float32


def convert_to_f32(raw, factor):
    """imDepth.convertTo(imDepth, CV_32F, factor) on any array of raw values (the whole image or the values read)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (raw.astype(F32) * F32(factor)).astype(F32)


def depth_at_points(xy, x_un, depth_img, factor, bf, convert_whole_image=False):
    """ComputeStereoFromRGBD: xy = mvKeys' (x, y), x_un = mvKeysUn's x; -> (mvuRight, mvDepth) float32.  A point whose truncated
    coordinates leave the image gets -1 (undefined in the reference)."""
    xy = np.asarray(xy, F32).reshape(-1, 2)
    x_un = np.asarray(x_un, F32).reshape(-1)
    h, w = depth_img.shape
    n = len(xy)
    ur = np.full(n, -1, F32); dp = np.full(n, -1, F32)
    conv = needs_convert(depth_img.dtype, factor)
    img = depth_img
    if conv and convert_whole_image:
        img = convert_to_f32(depth_img, factor)
    bf = F32(bf)
    for i in range(n):
        u, v = xy[i]
        if not (u > -1 and v > -1 and u < w and v < h):          # (NaN fails too)
            continue
        col, row = int(u), int(v)                                 # C's float -> int: towards zero
        d = img[row, col]
        if conv and not convert_whole_image:
            d = convert_to_f32(np.array([d]), factor)[0]
        d = F32(d)
        if d > 0:
            dp[i] = d
            with np.errstate(over="ignore"):
                ur[i] = F32(x_un[i] - F32(bf / d))
    return ur, dp


def rgbd_frame(image, depth_img, cam, bf, depth_factor, dist=None, rgb_order=False, n_features=1000, n_levels=8, scale_factor=1.2):
    """What GrabImageRGBD + Frame::Frame(RGB-D) leave behind: gray, mvKeys (lapping area {0, 0}: the stereo-left order), mvKeysUn,
    mDescriptors, mvuRight, mvDepth, the image bounds and the frame view whose grid is AssignFeaturesToGrid's.  cam = (fx, fy, cx, cy,
    bf, b) as Scene.frame_view_params gives it."""
    gray = image if image.ndim == 2 else gray_from_color(image, rgb_order)
    gray = np.ascontiguousarray(gray)
    h, w = gray.shape
    oe = ob.Extractor(n_features=n_features, max_width=w, max_height=h)
    rc, kps, desc, nmono = oe.extract(gray, (0, 0))
    assert rc == 0
    cam4 = cam[:4]
    kun = ob.undistort_keypoints(kps, cam4, dist)
    bounds = ob.image_bounds(w, h, cam4, dist)
    ur, dp = depth_at_points(np.stack([kps["x"], kps["y"]], axis=1), kun["x"], depth_img, depth_factor, bf)
    fv, keep = views.frame_view(kun, desc, ur, dp, bounds, cam, n_levels, scale_factor)
    return dict(gray=gray, kps=kps, kps_un=kun, desc=desc, uright=ur, depth=dp, bounds=bounds, fv=fv, keep=keep, n_mono=nmono)
