# Model section of the continuous detection configuration (values follow the reference's
# configs/detection/cont-det3d_8xb1_embodiedscan-3d-284class-9dof.py:17-58, which embodiedscan_amd.config.load_config also reads
# unchanged).  Frames 1 .. N of a walk-through, one set of detections per prefix (Embodied3DDetector).
n_points = 100000
model = dict(
    type='Embodied3DDetector',
    data_preprocessor=dict(type='Det3DDataPreprocessor', mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375],
                           bgr_to_rgb=True, pad_size_divisor=32, batchwise_inputs=True),
    backbone=dict(type='mmdet.ResNet', depth=50, base_channels=16, num_stages=4, out_indices=(0, 1, 2, 3),
                  frozen_stages=1, norm_cfg=dict(type='BN', requires_grad=False), norm_eval=True, style='pytorch'),
    backbone_3d=dict(type='MinkResNet', in_channels=3, depth=34),
    use_xyz_feat=True,
    bbox_head=dict(type='FCAF3DHeadRotMat', in_channels=(128, 256, 512, 1024), out_channels=128, voxel_size=.01,
                   pts_prune_threshold=20000, pts_assign_threshold=27, pts_center_threshold=18, num_classes=284,
                   num_reg_outs=12, center_loss=dict(type='mmdet.CrossEntropyLoss', use_sigmoid=True),
                   bbox_loss=dict(type='BBoxCDLoss', mode='l1', loss_weight=1.0, group='g8'),
                   cls_loss=dict(type='mmdet.FocalLoss'), decouple_bbox_loss=True, decouple_groups=4,
                   decouple_weights=[0.2, 0.2, 0.2, 0.4]),
    coord_type='DEPTH', train_cfg=dict(), test_cfg=dict(nms_pre=1000, iou_thr=.5, score_thr=.01))
optim_wrapper = dict(type='OptimWrapper', optimizer=dict(type='AdamW', lr=0.0002, weight_decay=0.0001),
                     clip_grad=dict(max_norm=10, norm_type=2))
# data section of the reference config (:134-190): no top-level PointSample (the slices of save_slices=True would cut a re-drawn
# cloud), per-frame instance visibility loaded, ConstructMultiSweeps behind the 3-D augmentation; `metainfo` is passed by the caller
_views = [dict(type='LoadImageFromFile', backend_args=None), dict(type='LoadDepthFromFile', backend_args=None),
          dict(type='ConvertRGBDToPoints', coord_type='CAMERA'), dict(type='PointSample', num_points=n_points // 10),
          dict(type='Resize', scale=(480, 480), keep_ratio=False)]
_load = dict(type='LoadAnnotations3D', with_visible_instance_masks=True)
_agg = dict(type='AggregateMultiViewPoints', coord_type='DEPTH', save_slices=True)
_pack = dict(type='Pack3DDetInputs', keys=['img', 'points', 'gt_bboxes_3d', 'gt_labels_3d'])
train_pipeline = [
    _load, dict(type='MultiViewPipeline', n_images=10, transforms=_views), _agg,
    dict(type='RandomFlip3D', sync_2d=False, flip_2d=False, flip_ratio_bev_horizontal=0.5, flip_ratio_bev_vertical=0.5),
    dict(type='GlobalRotScaleTrans', rot_range=[-0.087266, 0.087266], scale_ratio_range=[.9, 1.1],
         translation_std=[.1, .1, .1], shift_height=False),
    dict(type='ConstructMultiSweeps'), _pack]
test_pipeline = [_load, dict(type='MultiViewPipeline', n_images=50, ordered=True, transforms=_views), _agg,
                 dict(type='ConstructMultiSweeps'), _pack]
train_dataloader = dict(batch_size=1, num_workers=1, sampler=dict(type='DefaultSampler', shuffle=True),
                        dataset=dict(type='EmbodiedScanDataset', data_root='data', ann_file='embodiedscan_infos_train.pkl',
                                     pipeline=train_pipeline, test_mode=False, filter_empty_gt=True,
                                     box_type_3d='Euler-Depth'))
